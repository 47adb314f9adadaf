"""GPU: proving a chain from its checkpoints.  The inverse-walk kernel (vdf_minroot_inverse_walk / vdf_minroot_check_batch)
against oracle/pasta.py and against the host's forward evaluator, and the checkpoint circuits built on it
(vdf_nova_circuits_from_checkpoints / _materialize / _release, the windowed prove_recursively) against the path that carries
traces: every comparison is of bytes -- field arithmetic in canonical Montgomery form has no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pasta as o
from util import dev, dev_read, host, host_trace, mont_states, states_array
from vdf_amd._lib import lib
from vdf_amd.hip import VdfError
from vdf_amd.minroot import EvalMode, PallasVDF, State, VestaVDF, FIELD_FP, FIELD_FQ, nova_lib
from vdf_amd.nova import (CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_REFERENCE, InverseMinRootCircuit, NovaVDFProof, public_params)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = EvalMode.LTRAddChainSequential
FILL = 0xA5


# ---- the kernel against the oracle -------------------------------------------------------------------------------

@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_walk_against_the_oracle(ctx, field, n):
    rounds, m = 257, o.modulus(field)
    stride = rounds + 3                                   # walk_stride > rounds + 1: a gap of two entries between the runs
    rows = [(o.rand_fe(1000 + n, 3 * w, m), o.rand_fe(1000 + n, 3 * w + 1, m), o.rand_fe(1000 + n, 3 * w + 2, m)) for w in range(n)]
    start = mont_states(rows, m)
    want_trace = np.full((n, stride, 8), FILL * 0x0101010101010101, dtype="<u8")
    want_land, stood = [], []
    for w, r in enumerate(rows):
        s = o.State(*r)
        for k in range(rounds):                           # the state before round k goes to entry top - k = rounds - k
            stood.append((s.x, s.y, 0))
            s = o.minroot_inverse_round(s, field)
        want_land.append((s.x, s.y, s.i))
    want_trace[:, 1:rounds + 1] = mont_states(stood, m)[:, :8].reshape(n, rounds, 8)[:, ::-1]
    want_land = mont_states(want_land, m)
    d_states = dev(start)
    d_trace = dev(np.full((n, stride, 8), FILL * 0x0101010101010101, dtype="<u8"))
    ctx.minroot_inverse_walk(field, d_states, n, rounds, d_trace, walk_stride=stride, top=rounds)
    assert np.array_equal(host(d_states).reshape(n, 12), want_land)
    got = host(d_trace).reshape(n, stride, 8)
    # entry 0 of a run is the landing state's slot: untouched, like the gap behind the run
    assert np.all(got[:, 0] == FILL * 0x0101010101010101) and np.all(got[:, rounds + 1:] == FILL * 0x0101010101010101)
    assert np.array_equal(got, want_trace)
    # no trace: the same landing states
    d2 = dev(start)
    ctx.minroot_inverse_walk(field, d2, n, rounds)
    assert np.array_equal(host(d2).reshape(n, 12), want_land)


def test_walk_groups_lay_steps_out_trace_after_trace(ctx):
    """group / group_stride: walks of `every` rounds tile entries 1 .. t of their step's trace, steps t + 1 entries apart"""
    t, every, steps, m = 24, 8, 3, o.Q
    per = t // every
    tr = o.minroot_eval_trace(o.State(o.rand_fe(3, 0, m), o.rand_fe(3, 1, m), 5), t * steps, FIELD_FQ)
    start = mont_states([(tr[s * t + (k + 1) * every].x, tr[s * t + (k + 1) * every].y, tr[s * t + (k + 1) * every].i)
                         for s in range(steps) for k in range(per)], m)
    d_states = dev(start)
    d_trace = dev(np.full((steps, t + 1, 8), FILL * 0x0101010101010101, dtype="<u8"))
    ctx.minroot_inverse_walk(FIELD_FQ, d_states, steps * per, every, d_trace, walk_stride=every, top=every, group=per, group_stride=t + 1)
    got = host(d_trace).reshape(steps, t + 1, 8)
    for s in range(steps):
        assert np.all(got[s, 0] == FILL * 0x0101010101010101)
        want = mont_states([(x.x, x.y, 0) for x in tr[s * t + 1: s * t + t + 1]], m)[:, :8]
        assert np.array_equal(got[s, 1:], want)
    land = mont_states([(tr[s * t + k * every].x, tr[s * t + k * every].y, tr[s * t + k * every].i) for s in range(steps) for k in range(per)], m)
    assert np.array_equal(host(d_states).reshape(-1, 12), land)
    # heads: entry 0 of every step's trace from the landing states
    ctx.minroot_trace_heads(d_states, steps, per, d_trace, t + 1)
    got = host(d_trace).reshape(steps, t + 1, 8)
    assert np.array_equal(got[:, 0], land[::per, :8])


def test_walk_refuses_what_it_cannot_do(ctx):
    d_states = dev(np.zeros((4, 12), dtype="<u8"))
    d_trace = dev(np.zeros((4, 16, 8), dtype="<u8"))
    with pytest.raises(VdfError):                                      # top < rounds - 1: would write below the run
        ctx.minroot_inverse_walk(FIELD_FQ, d_states, 4, 10, d_trace, walk_stride=16, top=8)
    with pytest.raises(VdfError):                                      # host memory
        ctx.minroot_inverse_walk(FIELD_FQ, np.zeros((4, 12), dtype="<u8"), 4, 1)
    with pytest.raises(VdfError):
        ctx.minroot_inverse_walk(7, d_states, 4, 1)
    with pytest.raises(VdfError):
        ctx.minroot_inverse_walk(FIELD_FQ, d_states, 4, (1 << 22) + 1)
    ctx.minroot_inverse_walk(FIELD_FQ, d_states, 0, 10)                 # n = 0 does nothing
    ctx.minroot_inverse_walk(FIELD_FQ, d_states, 4, 0, d_trace, walk_stride=16, top=0)
    assert not host(d_trace).any() and not host(d_states).any()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_cut_walks(ctx, field):
    """2^16 rounds as one call, as 64 calls of 1,024 and as calls of 1, 65,534 and 1: identical traces and states"""
    T, n, m = 1 << 16, 3, o.modulus(field)
    rows = [(o.rand_fe(77, 3 * w, m), o.rand_fe(77, 3 * w + 1, m), o.rand_fe(77, 3 * w + 2, m)) for w in range(n)]
    start = mont_states(rows, m)
    results = []
    for cuts in ([T], [1024] * 64, [1, T - 2, 1]):
        d_states, d_trace = dev(start), dev(np.full((n, T + 1, 8), FILL * 0x0101010101010101, dtype="<u8"))
        top = T
        for c in cuts:
            ctx.minroot_inverse_walk(field, d_states, n, c, d_trace, walk_stride=T + 1, top=top)
            top -= c
        results.append((host(d_states).copy(), host(d_trace).copy()))
    for st, tr in results[1:]:
        assert np.array_equal(st, results[0][0]) and np.array_equal(tr, results[0][1])
    V = PallasVDF if field == FIELD_FQ else VestaVDF
    for w in range(n):                                                 # and the host's inverse_eval lands where they do
        back = V.inverse_eval(State.from_ints(field, *rows[w]), T)
        assert states_array([back])[0].tobytes() == results[0][0].reshape(n, 12)[w].tobytes()
    tr = results[0][1].reshape(n, T + 1, 8)
    assert np.all(tr[:, 0] == FILL * 0x0101010101010101)
    assert np.array_equal(tr[:, T], start[:, :8])


@pytest.mark.parametrize("every", [1 << 16, 1 << 10])
def test_walk_against_the_forward_evaluator_at_full_size(ctx, every):
    t, steps = 1 << 16, 3
    vdf = PallasVDF.new_with_mode(FAST)
    s = State.from_ints(FIELD_FQ, 123, 0, 0)
    boundaries, traces = [s], []
    for _ in range(steps):
        s, tr = host_trace(vdf, s, t)
        boundaries.append(s)
        traces.append(tr)
    if every == t:
        states = boundaries                                            # the 4 boundary states
    else:
        states = vdf.eval_checkpoints(boundaries[0], t * steps, every)
        assert states[::t // every] == boundaries
    _z0, c = InverseMinRootCircuit.from_checkpoints(t, every, steps, states)
    assert c.materialize(ctx) == [0] * steps
    assert c.memory() == (steps, steps * (t + 1) * 64)
    for k in range(steps):                                             # circuit k is forward step steps - 1 - k
        got = dev_read(ctx, c.trace_ptr(k), (t + 1) * 64).reshape(t + 1, 8)
        assert np.array_equal(got, traces[steps - 1 - k])
    c.release()
    assert c.memory() == (0, 0)
    c.free()


# ---- check_batch ---------------------------------------------------------------------------------------------------

def test_check_batch(ctx):
    n, t = 200, 1000
    vdf = PallasVDF.new_with_mode(FAST)
    originals = [State.from_ints(FIELD_FQ, o.rand_fe(9, 2 * k, o.Q), o.rand_fe(9, 2 * k + 1, o.Q), k) for k in range(n)]
    results = [vdf.eval(s, t) for s in originals]

    def flip(s, which):
        b = [bytearray(s.x), bytearray(s.y), bytearray(s.i)]
        b[which][3] ^= 0x10
        return State(bytes(b[0]), bytes(b[1]), bytes(b[2]))
    wrong = {10: ("r", 0), 33: ("r", 1), 64: ("r", 2), 65: ("o", 0), 127: ("o", 1), 128: ("o", 2)}
    for k, (side, which) in wrong.items():
        if side == "r":
            results[k] = flip(results[k], which)
        else:
            originals[k] = flip(originals[k], which)
    originals[199] = originals[198]                                    # an original that belongs to its neighbour
    want = [PallasVDF.check(results[k], t, originals[k]) for k in range(n)]
    assert want.count(True) == 193 and [k for k in range(n) if not want[k]] == sorted(list(wrong) + [199])
    assert PallasVDF.check_batch(ctx, results, t, originals) == want                 # host buffers
    res, org = states_array(results), states_array(originals)
    import torch
    d_res, d_org = dev(res), dev(org)
    d_ok = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.minroot_check_batch(FIELD_FQ, d_res, d_org, n, t, d_ok)                      # device buffers
    assert [bool(v) for v in d_ok.cpu().numpy()] == want
    assert np.array_equal(host(d_res).reshape(n, 12), res)                            # the inputs are left as they were
    ok = np.full(4, 7, dtype=np.int32)
    ctx.minroot_check_batch(FIELD_FQ, res, org, 0, t, ok)                             # n = 0 does nothing
    assert list(ok) == [7] * 4
    assert PallasVDF.check_batch(ctx, [], t, []) == []


# ---- proofs over checkpoint circuits ---------------------------------------------------------------------------------

def chain(t, n, seed=42, i0=1):
    initial = State.from_ints(FIELD_FQ, o.rand_fe(seed, 0, o.Q), 0, i0)
    return initial


@pytest.mark.parametrize("kind", [CIRCUIT_MINROOT_REFERENCE, CIRCUIT_MINROOT_BOUND])
def test_proofs_are_the_same_bytes(ctx, kind):
    t, n = 24, 6
    initial = chain(t, n)
    vdf = PallasVDF.new()
    pp = public_params(ctx, t, kind)
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(vdf, t, n, initial)
    circuits.upload(ctx)
    base = NovaVDFProof.prove_recursively(pp, circuits, t, z0)
    want, want_wire = base.serialize(), base.compress(pp).serialize()
    zi = [initial.x, initial.y, initial.i]
    assert base.verify(pp, n, z0, zi)
    base.free()
    for every in (24, 8):
        states = vdf.eval_checkpoints(initial, t * n, every)
        for window in (2, 3, 6):
            z0c, cc = InverseMinRootCircuit.from_checkpoints(t, every, n, states)
            assert z0c == z0
            proof = NovaVDFProof.prove_recursively(pp, cc, t, z0c, window_steps=window)
            assert proof.serialize() == want, (every, window)
            assert proof.verify(pp, n, z0, zi)
            assert proof.compress(pp).serialize() == want_wire, (every, window)
            assert cc.memory() == (0, 0)                               # what the call built, it released
            proof.free(); cc.free()
    # the default window, and upload = materialize of everything: eval -> upload -> prove works with either kind of circuits
    z0c, cc = InverseMinRootCircuit.from_checkpoints(t, 8, n, states)
    p1 = NovaVDFProof.prove_recursively(pp, cc, t, z0c)
    assert p1.serialize() == want and cc.memory() == (0, 0)
    cc.upload(ctx)
    assert cc.memory() == (n, n * (t + 1) * 64)
    p2 = NovaVDFProof.prove_recursively(pp, cc, t, z0c)
    assert p2.serialize() == want and cc.memory() == (n, n * (t + 1) * 64)   # the caller's traces are left alone
    p1.free(); p2.free(); cc.free(); circuits.free(); pp.free()


def test_proof_is_the_same_bytes_at_full_size(ctx):
    t, n = 1 << 16, 4
    initial = chain(t, n)
    vdf = PallasVDF.new_with_mode(FAST)
    pp = public_params(ctx, t)
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(vdf, t, n, initial)
    circuits.upload(ctx)
    base = NovaVDFProof.prove_recursively(pp, circuits, t, z0)
    want = base.serialize()
    states = [circuits.states(n - 1)[1]] + [circuits.states(n - 1 - s)[0] for s in range(n)]      # the 5 boundary states
    base.free(); circuits.free()
    z0c, cc = InverseMinRootCircuit.from_checkpoints(t, t, n, states)
    proof = NovaVDFProof.prove_recursively(pp, cc, t, z0c, window_steps=2)
    assert z0c == z0 and proof.serialize() == want
    assert proof.verify(pp, n, z0, [initial.x, initial.y, initial.i])
    assert cc.memory() == (0, 0)
    proof.free(); cc.free(); pp.free()


def test_window_accounting(ctx):
    t, n, W = 1024, 40, 8
    initial = chain(t, n, seed=8)
    vdf = PallasVDF.new_with_mode(FAST)
    states = vdf.eval_checkpoints(initial, t * n, t)
    z0, cc = InverseMinRootCircuit.from_checkpoints(t, t, n, states)
    pp = public_params(ctx, t)
    per = (t + 1) * 64
    seen = []

    def poll():
        r, b = cc.memory()
        assert b == r * per
        seen.append(r)
    cc.materialize(ctx, 0, W)
    cc.materialize(ctx, W, W, wait=False)
    poll()
    proof = None
    for k in range(n):
        proof = NovaVDFProof.prove_step(pp, proof, cc, k, z0)
        poll()
        if (k + 1) % W == 0:
            cc.release(k + 1 - W, W)
            poll()
            if k + 1 + W < n:
                cc.materialize(ctx, k + 1 + W, min(W, n - (k + 1 + W)), wait=False)
                poll()
    assert max(seen) == 2 * W and seen[-1] == 0
    assert cc.memory() == (0, 0)
    assert proof.verify(pp, n, z0, [initial.x, initial.y, initial.i])
    # the same chain through the windowed prove_recursively: the same bytes
    again = NovaVDFProof.prove_recursively(pp, cc, t, z0, window_steps=W)
    assert again.serialize() == proof.serialize()
    proof.free(); again.free(); cc.free(); pp.free()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_wrong_checkpoint_is_found_where_it_is(ctx, where):
    t, n = 64, 5
    initial = chain(t, n, seed=21)
    vdf = PallasVDF.new()
    states = vdf.eval_checkpoints(initial, t * n, t)
    traces, s = [], initial
    for _ in range(n):
        s, tr = host_trace(vdf, s, t)
        traces.append(tr)
    j = {"first": 0, "middle": 2, "last": n}[where]
    x = bytearray(states[j].x)
    x[5] ^= 0x04
    bad_states = list(states)
    bad_states[j] = State(bytes(x), states[j].y, states[j].i)
    # forward state j ends forward step j - 1 and starts forward step j; circuit k is forward step n - 1 - k
    flagged = sorted(n - 1 - f for f in (j - 1, j) if 0 <= f < n)
    z0, cc = InverseMinRootCircuit.from_checkpoints(t, t, n, bad_states)
    with pytest.raises(VdfError) as e:
        cc.materialize(ctx)
    assert e.value.code == 1
    assert ("circuit %d:" % flagged[0]) in nova_lib.vdf_nova_last_error().decode()
    assert cc.last_bad == [1 if k in flagged else 0 for k in range(n)]
    assert cc.memory()[0] == n - len(flagged)
    for k in range(n):
        if k in flagged:
            assert cc.trace_ptr(k) is None
            continue
        got = dev_read(ctx, cc.trace_ptr(k), (t + 1) * 64).reshape(t + 1, 8)
        assert np.array_equal(got, traces[n - 1 - k])
    pp = public_params(ctx, t)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_step(pp, None, cc, flagged[0], z0)
    assert e.value.code == 1 and "not materialised" in str(e.value)
    cc.free(); pp.free()


def test_misuse(ctx):
    t, n = 24, 4
    initial = chain(t, n, seed=4)
    vdf = PallasVDF.new()
    states = vdf.eval_checkpoints(initial, t * n, 8)
    z0, cc = InverseMinRootCircuit.from_checkpoints(t, 8, n, states)
    pp = public_params(ctx, t)
    # release of a range never materialised: a no-op
    cc.release(0, n)
    assert cc.memory() == (0, 0)
    # prove_step(k) with k + 1 not resident
    cc.materialize(ctx, 0, 1)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_step(pp, None, cc, 0, z0)
    assert e.value.code == 1 and "trace of circuit 1 not materialised" in str(e.value)
    # materialize twice: the second is a no-op (the same trace, the same memory)
    p0 = cc.trace_ptr(0)
    cc.materialize(ctx, 0, 1)
    assert cc.trace_ptr(0) == p0 and cc.memory() == (1, (t + 1) * 64)
    cc.materialize(ctx, 0, 2)
    assert cc.trace_ptr(0) == p0 and cc.memory() == (2, 2 * (t + 1) * 64)
    proof = NovaVDFProof.prove_step(pp, None, cc, 0, z0)              # now it goes
    assert proof.num_steps() == 1
    # out of range
    with pytest.raises(VdfError):
        cc.materialize(ctx, 3, 2)
    # circuits that carry their traces have upload, not materialize
    _z, full = InverseMinRootCircuit.eval_and_make_circuits(vdf, t, n, initial)
    with pytest.raises(VdfError):
        full.materialize(ctx)
    proof.free(); full.free(); cc.free(); pp.free()


def test_uploaded_traces_stay_through_release(ctx):
    """Circuits that carry host traces: upload gives every circuit a device trace of its own, release lets go of walked traces
    only and so leaves these where they are, and free takes them with the handle.  Every comparison is exact."""
    t, n = 4, 2
    per = (t + 1) * 64
    vdf = PallasVDF.new()
    initial = chain(t, n, seed=13)
    traces, s = [], initial
    for _ in range(n):
        s, tr = host_trace(vdf, s, t)
        traces.append(tr)
    _z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(vdf, t, n, initial)
    circuits.upload(ctx)
    assert circuits.memory() == (2, 2 * 5 * 64)
    ptrs = [circuits.trace_ptr(k) for k in range(n)]
    assert all(ptrs) and ptrs[0] != ptrs[1]
    circuits.release(0, 2)
    assert circuits.memory() == (2, 2 * 5 * 64) and [circuits.trace_ptr(k) for k in range(n)] == ptrs
    for k in range(n):                                                 # circuit k is forward step n - 1 - k
        assert np.array_equal(dev_read(ctx, ptrs[k], per).reshape(t + 1, 8), traces[n - 1 - k])
    circuits.upload(ctx)
    assert circuits.memory() == (2, 2 * 5 * 64) and [circuits.trace_ptr(k) for k in range(n)] == ptrs
    circuits.free()
    _z0, again = InverseMinRootCircuit.eval_and_make_circuits(vdf, t, n, initial)
    again.upload(ctx)
    assert again.memory() == (2, 2 * 5 * 64)
    again.free()


def test_a_window_that_cannot_fit(ctx):
    t = 1 << 18
    free = C.c_size_t(0)
    assert lib.vdf_dev_mem_info(ctx.handle, C.byref(free), None) == 0
    n = free.value // ((t + 1) * 64) + 2
    i0 = 3
    zero = bytes(32)
    states = [State(zero, zero, int(o.to_mont(i0 + k * t, o.Q)).to_bytes(32, "little")) for k in range(n + 1)]
    states[n] = PallasVDF.new_with_mode(FAST).eval(states[n - 1], t)   # circuit 0 (the last step) is a real one; the others never walk
    _z0, cc = InverseMinRootCircuit.from_checkpoints(t, t, n, states)
    cc.materialize(ctx, 0, 1)
    before = cc.memory()
    assert before == (1, (t + 1) * 64)
    with pytest.raises(VdfError) as e:
        cc.materialize(ctx, 0, n)
    assert e.value.code == 5                                           # VDF_ERR_OOM
    assert cc.memory() == before
    cc.free()


def test_c_example_runs_as_a_fresh_process():
    exe = os.path.join(ROOT, "examples", "prove_from_checkpoints")
    assert os.path.exists(exe), "examples/prove_from_checkpoints is built by vdf_amd/csrc/Makefile (all)"
    for args in (["6", "7", "6", "2"], ["6", "5", "3", "3"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "verify: true" in r.stdout and "traces left on the device: 0 steps, 0 bytes" in r.stdout


@pytest.mark.parametrize("args, launch", [(["6", "7", "4", "3"], 3), (["6", "7", "6", "2"], 5)])
def test_c_example_walks_in_many_launches_through_the_pump(args, launch):
    """A launch length below `every` (VDF_NOVA_WALK_LAUNCH, read once per process: hence a child): the first enqueue of a window's
    job no longer finishes it, and the rest of its rounds is what every prove_step's pump shares out -- t = 64 with `every` = 16
    in launches of 3 (six per job, windows of three steps), and `every` = 64 in launches of 5 (thirteen, windows of two).  The
    example exits 0 only if the proof verifies, which one over a wrongly rebuilt trace does not, and no trace is left resident."""
    exe = os.path.join(ROOT, "examples", "prove_from_checkpoints")
    assert os.path.exists(exe), "examples/prove_from_checkpoints is built by vdf_amd/csrc/Makefile (all)"
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=dict(os.environ, VDF_NOVA_WALK_LAUNCH=str(launch)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "verify: true" in r.stdout and "traces left on the device: 0 steps, 0 bytes" in r.stdout
