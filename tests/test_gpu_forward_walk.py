"""GPU: forward MinRoot walks, one lane per chain (vdf_minroot_forward_walk / vdf_minroot_eval_batch, vdf_amd/csrc/minroot.hip
k_forward_walk).  The reference for every comparison is the HOST evaluator (vdf_minroot_eval / vdf_minroot_eval_checkpoints of
libvdf_nova.so) and every comparison is of bytes: states, checkpoints and trace entries are canonical Montgomery residues, which
have no tolerance.  Then the walks' checkpoints into the prover (forward circuits), a walk beside a prover, and the plain-C
client examples/eval_farm."""
import ctypes as C
import os
import subprocess
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import vdf_amd
from oracle import pasta as o
from util import dev, host
from vdf_amd import _lib
from vdf_amd._lib import lib
from vdf_amd.hip import VdfError
from vdf_amd.minroot import EvalMode, PallasVDF, State, VestaVDF, FIELD_FP, FIELD_FQ, _State, nova_lib
from vdf_amd.nova import CIRCUIT_MINROOT_FORWARD, ForwardCircuits, NovaVDFProof, public_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = EvalMode.LTRAddChainSequential
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
CAP = _lib.MINROOT_FORWARD_MAX_ROUNDS
POOL = ThreadPoolExecutor(max_workers=16)                  # the host evaluator releases the GIL (ctypes)


def vdf_of(field):
    return (PallasVDF if field == FIELD_FQ else VestaVDF).new_with_mode(FAST)


def raw_states(rows):
    """[(x, y, i) Montgomery residues as ints] -> uint64[n, 12]"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for r in rows for v in r), dtype="<u8").reshape(-1, 12).copy()


def state_of(row):
    b = row.tobytes()
    return State(b[0:32], b[32:64], b[64:96])


def edge_rows(m):
    """Montgomery residues: x + y = 0 (mod m); x = y = 0; every limb all-ones below m (2^254 - 1); i = m - 1 (in value)"""
    a = o.rand_fe(31, 0, m)
    ones = (1 << 254) - 1
    return [(o.to_mont(a, m), o.to_mont(m - a, m), o.to_mont(9, m)),
            (0, 0, o.to_mont(4, m)),
            (ones, ones, ones),
            (o.to_mont(o.rand_fe(31, 1, m), m), o.to_mont(o.rand_fe(31, 2, m), m), o.to_mont(m - 1, m))]


def start_rows(field, n, seed, turn=0):
    m = o.modulus(field)
    e = edge_rows(m)
    e = e[turn % 4:] + e[:turn % 4]
    rnd = [tuple(o.to_mont(o.rand_fe(seed, 3 * w + k, m), m) for k in range(3)) for w in range(max(0, n - len(e)))]
    return raw_states((e + rnd)[:n])


def host_eval(field, row, rounds):
    """(final state uint64[12], trace uint64[rounds + 1, 8]) of vdf_minroot_eval"""
    buf = np.zeros((rounds + 1, 8), dtype="<u8")
    out = _State()
    assert nova_lib.vdf_minroot_eval(field, int(FAST), C.byref(state_of(row)._c()), rounds, C.byref(out), buf.ctypes.data) == 0
    return np.frombuffer(bytes(out), dtype="<u8").copy(), buf


def host_checkpoints(field, row, rounds, every):
    """uint64[rounds / every + 1, 12] of vdf_minroot_eval_checkpoints"""
    out = np.zeros((rounds // every + 1, 12), dtype="<u8")
    assert nova_lib.vdf_minroot_eval_checkpoints(field, int(FAST), C.byref(state_of(row)._c()), rounds, every, out.ctypes.data) == 0
    return out


# ---- 1. exact against the host ---------------------------------------------------------------------------------------

EVERY_FOR = {1: 1, 2: 1, 5: 5, 64: 16, 257: 1}


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_walk_equals_the_host_evaluator(ctx, field, n):
    for turn, rounds in enumerate([1, 2, 5, 64, 257]):
        every = EVERY_FOR[rounds]
        K = rounds // every
        start = start_rows(field, n, 100 * n + rounds, turn)
        stride, cps = rounds + 3, K + 2                      # a gap behind every run: entries the walk must leave alone
        d_states = dev(start)
        d_trace = dev(np.full((n, stride, 8), FILL, dtype="<u8"))
        d_cp = dev(np.full((n, cps, 12), FILL, dtype="<u8"))
        ctx.minroot_forward_walk(field, d_states, n, rounds, d_cp, every, cps, d_trace, stride, 0)
        finals = list(POOL.map(lambda w: host_eval(field, start[w], rounds), range(n)))
        want_cp = list(POOL.map(lambda w: host_checkpoints(field, start[w], rounds, every), range(n)))
        got_states, got_trace, got_cp = host(d_states).reshape(n, 12), host(d_trace).reshape(n, stride, 8), host(d_cp).reshape(n, cps, 12)
        assert np.array_equal(got_states, np.stack([f[0] for f in finals])), (n, rounds)
        assert np.array_equal(got_trace[:, 1:rounds + 1], np.stack([f[1][1:] for f in finals])), (n, rounds)
        assert np.all(got_trace[:, 0] == FILL) and np.all(got_trace[:, rounds + 1:] == FILL)
        assert np.array_equal(got_cp[:, 1:K + 1], np.stack([c[1:] for c in want_cp])), (n, rounds)
        assert np.all(got_cp[:, 0] == FILL) and np.all(got_cp[:, K + 1:] == FILL)
        # states only: the same landing states
        d2 = dev(start)
        ctx.minroot_forward_walk(field, d2, n, rounds)
        assert np.array_equal(host(d2).reshape(n, 12), got_states)


# ---- 2. resuming -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_a_cut_walk_is_the_same_walk(ctx, field):
    """300 rounds in one call and cut as 1 + 7 + 292: states, trace and checkpoints alike (every = 7 divides no cut but the
    second), and what the host gives"""
    T, n, every = 300, 70, 7
    K = T // every                                          # 42 checkpoints, the last after round 294
    start = start_rows(field, n, 5)
    results = []
    for cuts in ([T], [1, 7, 292]):
        d_states = dev(start)
        d_trace = dev(np.full((n, T + 2, 8), FILL, dtype="<u8"))
        d_cp = dev(np.full((n, K + 2, 12), FILL, dtype="<u8"))
        base = 0
        for c in cuts:
            ctx.minroot_forward_walk(field, d_states, n, c, d_cp, every, K + 2, d_trace, T + 2, base)
            base += c
        results.append((host(d_states).copy(), host(d_trace).copy(), host(d_cp).copy()))
    for a, b in zip(results[0], results[1]):
        assert np.array_equal(a, b)
    st, tr, cp = results[0][0].reshape(n, 12), results[0][1].reshape(n, T + 2, 8), results[0][2].reshape(n, K + 2, 12)
    assert np.all(tr[:, 0] == FILL) and np.all(tr[:, T + 1] == FILL) and np.all(cp[:, 0] == FILL) and np.all(cp[:, K + 1] == FILL)
    finals = list(POOL.map(lambda w: host_eval(field, start[w], T), range(n)))
    assert np.array_equal(st, np.stack([f[0] for f in finals]))
    assert np.array_equal(tr[:, 1:T + 1], np.stack([f[1][1:] for f in finals]))
    want_cp = list(POOL.map(lambda w: host_checkpoints(field, start[w], K * every, every), range(n)))
    assert np.array_equal(cp[:, 1:K + 1], np.stack([c[1:] for c in want_cp]))


# ---- 3. at scale -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_2_16_chains_checked_by_the_inverse_walk(ctx, field):
    import torch
    n, rounds = 1 << 16, 256
    rng = np.random.default_rng(16 + field)
    start = rng.integers(0, 2**64, size=(n, 3, 4), dtype=np.uint64)
    start[:, :, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)          # below 2^254 < m: every such word is a canonical Montgomery residue
    start = start.reshape(n, 12)
    d_start, d_states = dev(start), dev(start)
    ctx.minroot_forward_walk(field, d_states, n, rounds)
    d_ok = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.minroot_check_batch(field, d_states, d_start, n, rounds, d_ok)
    assert int(d_ok.sum().item()) == n and int(d_ok.min().item()) == 1
    got = host(d_states).reshape(n, 12)
    picks = [0, 1, 63, 64, 65, n - 1] + [int(v) for v in rng.integers(0, n, size=26)]
    want = list(POOL.map(lambda w: host_eval(field, start[w], rounds)[0], picks))
    assert np.array_equal(got[picks], np.stack(want))
    # one byte of one output: exactly that chain is rejected
    victim = 40000
    bad = got.copy()
    bad.view(np.uint8).reshape(n, 96)[victim, 37] ^= 0x20
    d_bad = dev(bad)
    ctx.minroot_check_batch(field, d_bad, d_start, n, rounds, d_ok)
    ok = d_ok.cpu().numpy()
    assert ok[victim] == 0 and int(ok.sum()) == n - 1


# ---- 4. eval_batch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_eval_batch(ctx, field):
    n, T, every = 130, 256, 32
    per = T // every + 1
    start = start_rows(field, n, 44)
    want = np.stack(list(POOL.map(lambda w: host_checkpoints(field, start[w], T, every), range(n))))     # [n, per, 12]
    outs = []
    for launch in (256, 64, 0):                                            # one launch, four launches, the default
        out = np.full((n, per, 12), FILL, dtype="<u8")
        ctx.minroot_eval_batch(field, start, n, T, out, every=every, launch_rounds=launch)           # host pointers
        outs.append(out)
        d_init, d_out = dev(start), dev(np.full((n, per, 12), FILL, dtype="<u8"))
        ctx.minroot_eval_batch(field, d_init, n, T, d_out, every=every, launch_rounds=launch)        # device pointers
        ctx.sync()
        assert np.array_equal(host(d_out).reshape(n, per, 12), out), launch
        assert np.array_equal(host(d_init).reshape(n, 12), start)                                     # left as it was
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and np.array_equal(outs[0], want)
    # every = 0: final states only
    fin = np.full((n, 12), FILL, dtype="<u8")
    ctx.minroot_eval_batch(field, start, n, T, fin, launch_rounds=64)
    assert np.array_equal(fin, want[:, -1])
    d_fin = dev(np.full((n, 12), FILL, dtype="<u8"))
    ctx.minroot_eval_batch(field, dev(start), n, T, d_fin)
    ctx.sync()
    assert np.array_equal(host(d_fin).reshape(n, 12), want[:, -1])
    # the reference-named mirror
    V = PallasVDF if field == FIELD_FQ else VestaVDF
    some = [state_of(start[w]) for w in range(5)]
    assert V.eval_batch(ctx, some, T) == [state_of(want[w, -1]) for w in range(5)]
    assert V.eval_batch(ctx, some, T, every) == [[state_of(want[w, k]) for k in range(per)] for w in range(5)]
    assert V.eval_batch(ctx, [], T) == []
    with pytest.raises(ValueError):
        V.eval_batch(ctx, some, T, 7)


# ---- 5. what is refused ----------------------------------------------------------------------------------------------

def test_refusals_leave_the_states_alone(ctx):
    n = 8
    start = start_rows(FIELD_FQ, n, 3)
    d_states = dev(start)
    d_trace = dev(np.full((n, 16, 8), FILL, dtype="<u8"))
    d_cp = dev(np.full((n, 16, 12), FILL, dtype="<u8"))

    def untouched():
        return (np.array_equal(host(d_states).reshape(n, 12), start) and np.all(host(d_trace) == FILL) and np.all(host(d_cp) == FILL))
    bad_arg, bad_len = _lib.VDF_ERR_BAD_ARG, _lib.VDF_ERR_BAD_LENGTH
    for code, call in (
            (bad_arg, lambda: ctx.minroot_forward_walk(7, d_states, n, 4, d_cp, 2, 16, d_trace, 16, 0)),                      # field
            (bad_arg, lambda: ctx.minroot_forward_walk(FIELD_FQ, d_states, n, CAP + 1, d_cp, 2, 16, d_trace, 16, 0)),        # too long
            (bad_len, lambda: ctx.minroot_forward_walk(FIELD_FQ, d_states, (1 << 31) + 1, 4)),                                # n > 2^31
            (bad_arg, lambda: ctx.minroot_forward_walk(FIELD_FQ, start.copy(), n, 4)),                                        # host memory
            (bad_arg, lambda: ctx.minroot_forward_walk(FIELD_FQ, d_states, n, 4, np.zeros((n, 16, 12), dtype="<u8"), 2, 16)),
            (bad_arg, lambda: ctx.minroot_forward_walk(FIELD_FQ, d_states, n, 4, None, 0, 0, np.zeros((n, 16, 8), dtype="<u8"), 16)),
            (bad_arg, lambda: ctx.minroot_forward_walk(FIELD_FQ, d_states, n, 4, d_cp, 0, 16)),                               # checkpoints, no every
            (bad_arg, lambda: ctx.minroot_eval_batch(7, d_states, n, 8, d_cp)),
            (bad_arg, lambda: ctx.minroot_eval_batch(FIELD_FQ, d_states, n, 10, d_cp, every=4)),                              # 4 does not divide 10
            (bad_arg, lambda: ctx.minroot_eval_batch(FIELD_FQ, d_states, n, 8, d_cp, every=4, launch_rounds=CAP + 1)),
            (bad_len, lambda: ctx.minroot_eval_batch(FIELD_FQ, d_states, (1 << 31) + 1, 8, d_cp))):
        with pytest.raises(VdfError) as e:
            call()
        assert e.value.code == code
        assert untouched()
    # the cap itself is accepted by the argument check (no walk: n = 0), and n = 0 / rounds = 0 do nothing
    ctx.minroot_forward_walk(FIELD_FQ, d_states, 0, CAP, d_cp, 2, 16, d_trace, 16, 0)
    ctx.minroot_forward_walk(FIELD_FQ, d_states, n, 0, d_cp, 2, 16, d_trace, 16, 0)
    ctx.minroot_eval_batch(FIELD_FQ, d_states, 0, 8, d_cp, every=4)
    assert untouched()
    # rounds_total = 0: the chains stand where they started
    out = np.full((n, 12), FILL, dtype="<u8")
    ctx.minroot_eval_batch(FIELD_FQ, start, n, 0, out)
    assert np.array_equal(out, start)


# ---- 6. into the prover ----------------------------------------------------------------------------------------------

def test_device_checkpoints_into_the_forward_prover(ctx):
    """t = 2^10, 4 steps: the chain's checkpoints from the device (every = t and t / 4) -> forward circuits -> materialize ->
    prove -> verify -> compress; the wire bytes are those of the same chain evaluated by the host and pushed as traces"""
    t, steps = 1 << 10, 4
    vdf = PallasVDF.new_with_mode(FAST)
    initial = State.from_ints(FIELD_FQ, o.rand_fe(61, 0, o.Q), 0, 3)
    pp = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)
    z0, fc = ForwardCircuits.begin(t, initial)
    s = initial
    for _ in range(steps):
        s, tr = vdf.eval_with_trace(s, t)
        fc.push_trace(tr)
    base = NovaVDFProof.prove_recursively(pp, fc, t, z0)
    zi = [s.x, s.y, s.i]
    assert base.verify(pp, steps, z0, zi)
    want_running, snark = base.serialize(), base.compress(pp)
    want_wire = snark.serialize()
    snark.free(); base.free(); fc.free()
    others = [State.from_ints(FIELD_FQ, o.rand_fe(61, 1 + k, o.Q), 0, k) for k in range(3)]      # the chain is one of four on the device
    for every in (t, t // 4):
        per = t // every
        chains = PallasVDF.eval_batch(ctx, others[:1] + [initial] + others[1:], t * steps, every)
        cps = chains[1]
        assert cps[0] == initial and cps[-1] == s and len(cps) == steps * per + 1
        z0c, fcp = ForwardCircuits.begin(t, initial)
        for k in range(steps):
            fcp.push_checkpoints(every, cps[k * per:(k + 1) * per + 1])
        assert z0c == z0 and fcp.materialize(ctx) == [0] * steps
        proof = NovaVDFProof.prove_recursively(pp, fcp, t, z0c)
        assert proof.verify(pp, steps, z0, zi) and proof.serialize() == want_running
        sn = proof.compress(pp)
        assert sn.verify(pp, steps, z0, zi) and sn.serialize() == want_wire, every
        sn.free(); proof.free(); fcp.free()
    pp.free()


# ---- 7. beside a prover ----------------------------------------------------------------------------------------------

def test_a_walk_beside_a_prover_changes_no_proof(ctx):
    """a thread walks 2^14 chains on a second context, launch after launch, while this thread proves a chain: the proof's bytes
    are those of the solo run, and the walks' states those of a quiet device"""
    t, steps, n, rounds = 1 << 12, 6, 1 << 14, 64
    vdf = PallasVDF.new_with_mode(FAST)
    initial = State.from_ints(FIELD_FQ, 0xFEEDC0DE, 0, 0)
    pp = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)
    z0, fc = ForwardCircuits.begin(t, initial)
    s = initial
    for _ in range(steps):
        s, tr = vdf.eval_with_trace(s, t)
        fc.push_trace(tr)
    solo = NovaVDFProof.prove_recursively(pp, fc, t, z0)
    assert solo.verify(pp, steps, z0, [s.x, s.y, s.i])
    want = solo.serialize()
    solo.free()
    rng = np.random.default_rng(77)
    start = rng.integers(0, 2**64, size=(n, 3, 4), dtype=np.uint64)
    start[:, :, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    start = start.reshape(n, 12)
    side = vdf_amd.Context(0)
    try:
        quiet = dev(start)
        side.minroot_forward_walk(FIELD_FQ, quiet, n, rounds)
        quiet = host(quiet).copy()
        launches, errors, stop, d_states = [0], [], threading.Event(), dev(start)

        def walker():
            try:
                side.minroot_forward_walk(FIELD_FQ, d_states, n, rounds)
                launches[0] += 1
                scratch = dev(start)
                while not stop.is_set() and launches[0] < 200:
                    side.minroot_forward_walk(FIELD_FQ, scratch, n, rounds)
                    launches[0] += 1
            except Exception as ex:                                             # noqa: BLE001
                errors.append(ex)
        th = threading.Thread(target=walker)
        th.start()
        try:
            proofs = [NovaVDFProof.prove_recursively(pp, fc, t, z0) for _ in range(3)]
        finally:
            stop.set()
            th.join()
        assert not errors, errors
        assert launches[0] >= 1
        for p in proofs:
            assert p.serialize() == want
            p.free()
        assert np.array_equal(host(d_states), quiet)
    finally:
        side.close()
    fc.free(); pp.free()


# ---- 8. the plain-C client -------------------------------------------------------------------------------------------

def test_eval_farm_client():
    """examples/eval_farm as a fresh child process: 200 chains of 4 x 2^10 rounds with a checkpoint every 256 -- exit 0, one line
    per chain, every check ok, chains 0 and 199 proved, verified and equal to the host's evaluation"""
    exe = os.path.join(ROOT, "examples", "eval_farm")
    assert os.path.exists(exe), "examples/eval_farm is built by vdf_amd/csrc/Makefile (all)"
    r = subprocess.run([exe, "200", "10", "4", "8"], capture_output=True, text=True, timeout=600)      # a fresh child process
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ln.startswith("chain "))
    assert len(lines) == 200 and all(v.startswith("check: ok") for v in lines.values())
    for k in (0, 199):
        assert lines["chain %d" % k] == "check: ok; proved 4 steps, verify: true; final state equals the host's: yes"
    assert "200 chains, 0 failed their check" in r.stdout
