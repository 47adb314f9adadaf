"""GPU: powers by a caller-supplied addition chain in forward walk tapes (include/vdf_hip.h VDF_TAPE_POWC, kernel
k_tape_forward_walk_chain; include/vdf_nova.h vdf_cs_pow_chain).  The oracle throughout: a POWC of a chain with exponent E is byte
for byte a POW of E -- on the device (the unchanged k_tape_forward_walk), on the host (vdf_nova_forward_tape_eval) and over the
integers.

a. the MinRoot forward round with its root by the reference's chain equals vdf_minroot_forward_walk, landings, trace and
   checkpoints with guards: a partial wavefront, a full one, a second and a third workgroup; both fields; a root of zero;
b. a body of every op with powers by POW and by chains of different n_tmp equals the host evaluator and the integers;
c. the layout of forward_tape_spec with a POWC tape: nothing outside the runs is touched;
d. round_tape_eval_batch with the POWC tape equals vdf_minroot_eval_batch, host and device pointers;
e. the launcher's refusals, each followed by a valid call; the slot cap through n_tmp and the work cap, each exact at the cap;
f. which kernel a tape launches, by the context's event log;
g. the pipeline once: checkpoints by the POWC tape give the proof bytes the POW tape's give;
h. the plain-C example, as a fresh child process."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import pasta as o
from util import dev, host, mont_states
from rounds_spec import MOD, mont_rows
from walks_spec import GUARD, expected_bytes, guarded, minroot_body, start_entries, tape_ints
from forward_tape_spec import (CP_STRIDE, LAYOUT, LAYOUT_FRONT, LAYOUT_TRACE, layout_cp_entries, minroot_forward_body, model_forward,
                               root_exponent)
from pow_chain_spec import (ACC, NONE, TAPE_POWC, EVERY_OP_CHAINS_A, EVERY_OP_CHAINS_B, every_op_chain_body, every_op_chain_ints,
                            minroot_chain_body)
from test_gpu_custom_walk import chain, dguard, prove, window_by_walks
from test_pow_chain_host import chain_tape, invalid_chains, patch, wide_chain_body
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError, FORWARD_TAPE_MAX_WORK, WALK_MAX_SLOTS
from vdf_amd import minroot
from vdf_amd.nova import forward_tape_eval, pow_chain_window, record_forward_body, record_walk_body, FIELD_FP, FIELD_FQ

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I0 = 0xFEDCBA
FIELDS = [FIELD_FQ, FIELD_FP]


@functools.lru_cache(maxsize=None)
def minroot_tape(field, kind):
    """the MinRoot forward round as a tape: its root by POW, by the reference's chain, or by a window-4 chain"""
    if kind == "pow":
        return record_forward_body(minroot_forward_body(field), field)
    steps = minroot.pow_chain(field) if kind == "minroot" else pow_chain_window(root_exponent(field), 4)
    return record_forward_body(minroot_chain_body(field, steps), field)


def minroot_case(ctx, field, n, rounds, kind):
    m, every = MOD[field], {1: 1, 2: 1, 5: 5, 64: 16}[rounds]
    K, stride = rounds // every, rounds + 3
    cps = K + 2                                        # entries nobody writes behind every run of both arrays
    rng = np.random.default_rng(1000 * n + rounds + field)
    xy = rng.integers(1, 2**62, size=(n, 2))
    rows = [(int(xy[w, 0]) ** 4, int(xy[w, 1]) ** 3, I0 + 1000 * w) for w in range(n)]
    rows[0] = (5, m - 5, I0)                           # x + y = 0: the root of zero
    states = mont_states([[v % m for v in r] for r in rows], m)
    start = np.ascontiguousarray(states[:, :8])
    kw = dict(j_base=I0, j_walk_step=1000)
    d_states = dev(states)
    want_tr, want_cp = dguard(2 * (n * stride + 1)), dguard(3 * (n * cps + 1))
    ctx.minroot_forward_walk(field, d_states, n, rounds, want_cp, every, cps, want_tr, stride, 0)
    got = {}
    for k in (kind, "pow"):
        d_entries, d_tr, d_cp = dev(start), dguard(2 * (n * stride + 1)), dguard(2 * (n * cps + 1))
        ctx.round_tape_forward_walk(field, minroot_tape(field, k), None, d_entries, n, rounds, d_cp, every, cps, d_tr, stride, 0, **kw)
        got[k] = (d_entries, d_tr, d_cp)
    ctx.sync()
    entries, tr, cp = (host(x) for x in got[kind])
    # the built-in forward walk
    assert tr.tobytes() == host(want_tr).tobytes()
    gt = tr.reshape(-1, 8)
    assert int((gt[:, 0] != np.uint64(GUARD)).sum()) == n * rounds   # (a canonical x never has an all-ones limb)
    assert (gt[n * stride:] == np.uint64(GUARD)).all() and (gt[0] == np.uint64(GUARD)).all()
    gc, wc = cp.reshape(-1, 8), host(want_cp).reshape(-1, 12)
    assert gc.tobytes() == np.ascontiguousarray(wc[:, :8]).tobytes()      # (guards are all-ones on both sides)
    assert int((gc[:, 0] != np.uint64(GUARD)).sum()) == n * K
    assert entries.reshape(n, 8).tobytes() == np.ascontiguousarray(host(d_states).reshape(n, 12)[:, :8]).tobytes()
    # the POW tape through the unchanged kernel
    assert all(host(a).tobytes() == b.tobytes() for a, b in zip(got["pow"], (entries, tr, cp)))
    # the host evaluator over the POWC tape
    h_entries, h_tr, h_cp = start.copy().reshape(-1, 4), guarded(2 * (n * stride + 1)), guarded(2 * (n * cps + 1))
    forward_tape_eval(field, minroot_tape(field, kind), None, h_entries, n, rounds, h_cp, every, cps, h_tr, stride, 0, **kw)
    assert (h_entries.tobytes(), h_tr.tobytes(), h_cp.tobytes()) == (entries.tobytes(), tr.tobytes(), cp.tobytes())


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("rounds", [1, 2, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_a_minroot_tape_by_the_reference_chain_equals_the_forward_walk_kernel(ctx, n, rounds, field):
    minroot_case(ctx, field, n, rounds, "minroot")


@pytest.mark.parametrize("field", FIELDS)
def test_b_minroot_tape_by_a_window_chain(ctx, field):
    minroot_case(ctx, field, 65, 5, "window")


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("chains", [EVERY_OP_CHAINS_A, EVERY_OP_CHAINS_B], ids=["A", "B"])
@pytest.mark.parametrize("rounds", [1, 2, 5])
def test_a_body_of_every_op_with_powers_by_chains_on_the_device(ctx, rounds, chains, field):
    m, n = MOD[field], 65
    tape = record_forward_body(every_op_chain_body(field, chains), field)
    start = start_entries(n, 3, m, np.random.default_rng(field + rounds))
    assert {0, 1, m - 1} <= set(start)
    inv, kw = [m - 1], dict(walk_stride=rounds + 2, j_base=2**64 - 3, j_walk_step=1)
    n_tr = 3 * (n * (rounds + 2) + 1)
    d_entries, d_trace = dev(mont_rows(start, m)), dguard(n_tr)
    ctx.round_tape_forward_walk(field, tape, mont_rows(inv, m), d_entries, n, rounds, trace=d_trace, **kw)
    ctx.sync()
    entries, trace = mont_rows(start, m), guarded(n_tr)
    forward_tape_eval(field, tape, mont_rows(inv, m), entries, n, rounds, trace=trace, **kw)
    assert host(d_entries).tobytes() == entries.tobytes() and host(d_trace).tobytes() == trace.tobytes()
    land, tr = list(start), [None] * n_tr
    model_forward(every_op_chain_ints(chains), m, 3, inv, land, n, rounds, trace=tr, **kw)
    assert tape_ints(entries, m) == land and trace.tobytes() == expected_bytes(tr, m)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("every", [1, 2, 5])
def test_strides_base_every_and_the_counter_with_a_chain(ctx, every, field):
    m = MOD[field]
    tape = record_forward_body(every_op_chain_body(field, EVERY_OP_CHAINS_A), field)
    start, inv = start_entries(LAYOUT["n"], 3, m, np.random.default_rng(5 + field)), [0x1234567 % m]
    n_cp = layout_cp_entries(every)
    want_tr, want_cp = [None] * (3 * (LAYOUT_TRACE - LAYOUT_FRONT)), [None] * (3 * (n_cp - LAYOUT_FRONT))
    land = list(start)
    model_forward(every_op_chain_ints(EVERY_OP_CHAINS_A), m, 3, inv, land, checkpoints=want_cp, every=every, cp_stride=CP_STRIDE[every],
                  trace=want_tr, **LAYOUT)
    front = [None] * (3 * LAYOUT_FRONT)
    d_entries, d_tr, d_cp = dev(mont_rows(start, m)), dguard(3 * LAYOUT_TRACE), dguard(3 * n_cp)
    ctx.round_tape_forward_walk(field, tape, mont_rows(inv, m), d_entries, checkpoints=d_cp[3 * LAYOUT_FRONT:], every=every,
                                cp_stride=CP_STRIDE[every], trace=d_tr[3 * LAYOUT_FRONT:], **LAYOUT)
    ctx.sync()
    assert tape_ints(host(d_entries), m) == land
    assert host(d_tr).tobytes() == expected_bytes(front + want_tr, m) and host(d_cp).tobytes() == expected_bytes(front + want_cp, m)


@pytest.mark.parametrize("field", FIELDS)
def test_eval_batch_with_a_chain_equals_the_minroot_eval_batch(ctx, field):
    m, n, T = MOD[field], 65, 130
    tape = minroot_tape(field, "minroot")
    rng = np.random.default_rng(77 + field)
    xy = rng.integers(1, 2**62, size=(n, 2))
    states = mont_states([[int(xy[w, 0]) ** 4 % m, int(xy[w, 1]) ** 3 % m, I0 + 1000 * w] for w in range(n)], m)
    start = np.ascontiguousarray(states[:, :8])
    jk = dict(j_base=I0, j_walk_step=1000)
    for every in (0, 5, 65):
        per = T // every + 1 if every else 1
        want = np.zeros((n, per, 12), dtype="<u8")
        ctx.minroot_eval_batch(field, states, n, T, want, every=every)
        want = np.ascontiguousarray(want[:, :, :8])
        for launch in (0, 7):
            out = np.zeros((n, per, 8), dtype="<u8")
            ctx.round_tape_eval_batch(field, tape, None, start, n, T, out, every=every, launch_rounds=launch, **jk)      # host pointers
            assert out.tobytes() == want.tobytes(), (every, launch)
            d_init, d_out = dev(start), dev(np.zeros((n, per, 8), dtype="<u8"))
            ctx.round_tape_eval_batch(field, tape, None, d_init, n, T, d_out, every=every, launch_rounds=launch, **jk)  # device pointers
            ctx.sync()
            assert host(d_out).tobytes() == want.tobytes(), (every, launch)
            assert host(d_init).tobytes() == start.tobytes()                   # a device `initial` is left as it was


def test_the_launcher_refuses_a_bad_chain_and_the_context_goes_on(ctx):
    field, m = FIELD_FQ, o.Q
    steps = minroot.pow_chain(field)
    want = mont_rows([pow(3, root_exponent(field), m)], m)

    def valid():
        d = dev(mont_rows([3], m))
        ctx.round_tape_forward_walk(field, chain_tape(steps=steps), None, d, 1, 1)
        ctx.sync()
        assert host(d).tobytes() == want.tobytes()

    def refused(t):
        d = dev(mont_rows([3], m))
        with pytest.raises(VdfError) as e:
            ctx.round_tape_forward_walk(field, t, None, d, 1, 1)
        assert e.value.code == VDF_ERR_BAD_ARG
        with pytest.raises(VdfError) as e:
            ctx.round_tape_eval_batch(field, t, None, mont_rows([3], m), 1, 1, np.zeros((1, 4), dtype="<u8"))
        assert e.value.code == VDF_ERR_BAD_ARG
        ctx.sync()
        assert host(d).tobytes() == mont_rows([3], m).tobytes()
        valid()                                                 # a valid call right after it

    def broken(change):
        t = chain_tape(steps=steps)
        change(t)
        refused(t)
    valid()
    # every invalid chain of the CPU list, written into the constants of a tape that was valid
    for name, bad in invalid_chains():
        t = chain_tape(steps=[(0, 0, NONE, NONE)] * 95)         # 12 constants of room
        raw = bytes([len(bad), 12, 0, 0]) + bytes(v for s in bad for v in s)
        t.consts.view(np.uint8).reshape(-1)[:12 * 32] = np.frombuffer((raw + bytes(12 * 32))[:12 * 32], dtype=np.uint8)
        refused(t)
    broken(lambda t: patch(t, 0, 4, ACC))                       # step 0 from ACC
    broken(lambda t: patch(t, 0, 4, 1))                         # read before it is written
    broken(lambda t: patch(t, 0, 7, 9))                         # an index equal to n_tmp
    broken(lambda t: patch(t, 0, 1, 13))                        # n_tmp = 13
    broken(lambda t: patch(t, 0, 0, 96))                        # 96 steps
    broken(lambda t: patch(t, 0, 2, 1))
    broken(lambda t: patch(t, 4, 4, 1))                         # non-zero padding
    broken(lambda t: patch(t, 4, 31, 1))
    broken(lambda t: patch(t, 1, 4 + 4 * 11 + 1 - 32, 255))     # step 11: 255 squarings: the exponent passes 2^256
    broken(lambda t: setattr(t.c, "n_consts", 4))               # the chain runs past n_consts
    broken(lambda t: setattr(t.ops[1], "b", 5))
    broken(lambda t: setattr(t.ops[1], "a", 1))                 # a POWC of a slot nothing wrote
    t = chain_tape(steps=steps)
    patch(t, 0, 1, 12)                                          # n_tmp = 12 declared is accepted
    d = dev(mont_rows([3], m))
    ctx.round_tape_forward_walk(field, t, None, d, 1, 1)
    ctx.sync()
    assert host(d).tobytes() == want.tobytes()
    # a POWC in vdf_round_tape_run and in vdf_round_tape_walk
    inv, start4 = mont_rows([5], m), mont_rows(list(range(1, 9)), m)
    d_entries, d_out = dev(start4), dguard(8)
    w = record_walk_body(minroot_body(field), field)
    ctx.round_tape_walk(field, w, inv, dev(start4), 4, 1)
    mul = next(i for i, x in enumerate(w.op_list()) if x[0] == 6)
    w.ops[mul].op, w.ops[mul].b = TAPE_POWC, 0
    w.consts[0] = chain_tape().consts[0]
    w.c.n_consts = 1
    with pytest.raises(VdfError) as e:
        ctx.round_tape_walk(field, w, inv, d_entries, 4, 1)
    assert e.value.code == VDF_ERR_BAD_ARG
    with pytest.raises(VdfError) as e:
        ctx.round_tape_run(field, chain_tape(), 4, None, d_entries, d_out)
    assert e.value.code == VDF_ERR_BAD_ARG
    ctx.sync()
    assert host(d_entries).tobytes() == start4.tobytes() and (host(d_out) == np.uint64(GUARD)).all()
    valid()


def test_the_slot_cap_through_the_temporaries_runs_and_one_beyond_is_refused(ctx):
    """n_slots + 2 n_adv + n_tmp = 21 + 11 = 32 is 64 KiB of LDS: it launches and is exact; 21 + 12 is refused before a launch"""
    field, m, n, rounds, na = FIELD_FQ, o.Q, 65, 3, 5
    body, live = wide_chain_body(11)
    tape = record_forward_body(body, field)
    assert tape.c.n_slots + 2 * na + 11 == WALK_MAX_SLOTS
    start = start_entries(n, na, m, np.random.default_rng(9))
    d_entries, entries = dev(mont_rows(start, m)), mont_rows(start, m)
    ctx.round_tape_forward_walk(field, tape, None, d_entries, n, rounds)
    ctx.sync()
    forward_tape_eval(field, tape, None, entries, n, rounds)
    assert host(d_entries).tobytes() == entries.tobytes()
    land = list(start)
    model_forward(lambda cur, j, inv, mm: [pow((cur[0] + j) * (2**live - 1), 4, mm)] * na, m, na, [], land, n, rounds)
    assert tape_ints(entries, m) == land
    patch(tape, 0, 1, 12)                                       # the same chain with 12 temporaries declared: 33 slots
    with pytest.raises(VdfError) as e:
        ctx.round_tape_forward_walk(field, tape, None, d_entries, n, rounds)
    assert e.value.code == VDF_ERR_BAD_ARG
    ctx.sync()
    assert host(d_entries).tobytes() == entries.tobytes()


def test_the_work_cap_of_a_chain_runs_and_one_beyond_is_refused(ctx):
    """255 squarings and one product per round: 4,096 rounds are exactly VDF_FORWARD_TAPE_MAX_WORK = 2^20 products in one launch"""
    field, m = FIELD_FQ, o.Q
    tape = chain_tape(steps=[(0, 255, 0, NONE)])
    rounds = FORWARD_TAPE_MAX_WORK // 256
    assert rounds * 256 == FORWARD_TAPE_MAX_WORK
    d_entries, entries = dev(mont_rows([3], m)), mont_rows([3], m)
    with pytest.raises(VdfError) as e:
        ctx.round_tape_forward_walk(field, tape, None, d_entries, 1, rounds + 1)
    assert e.value.code == VDF_ERR_BAD_ARG
    ctx.sync()
    assert host(d_entries).tobytes() == entries.tobytes()
    ctx.round_tape_forward_walk(field, tape, None, d_entries, 1, rounds)
    ctx.sync()
    forward_tape_eval(field, tape, None, entries, 1, rounds)
    assert host(d_entries).tobytes() == entries.tobytes()
    assert tape_ints(entries, m) == [pow(3, pow(2**255 + 1, rounds, m - 1), m)]


def test_which_kernel_a_tape_launches(ctx):
    """a tape without a POWC launches k_tape_forward_walk as before, one with it k_tape_forward_walk_chain (an event's name holds
    the first 23 characters)"""
    field, m = FIELD_FQ, o.Q
    d = dev(mont_rows([3, 4], m))
    try:
        ctx.set_kernel_timing(True)
        ctx.kernel_events()
        ctx.round_tape_forward_walk(field, minroot_tape(field, "pow"), None, d, 1, 1)
        ctx.round_tape_forward_walk(field, minroot_tape(field, "minroot"), None, d, 1, 1)
        ctx.round_tape_forward_walk(field, minroot_tape(field, "pow"), None, d, 1, 1)
        ctx.sync()
        names = [e[0] for e in ctx.kernel_events()]
        assert names == ["k_tape_forward_walk", "k_tape_forward_walk_chain"[:23], "k_tape_forward_walk"]
    finally:
        ctx.set_kernel_timing(False)


def test_the_pipeline_with_checkpoints_by_a_chain_tape(ctx):
    """checkpoints by round_tape_eval_batch over the POWC tape, advice by round_tape_walk, three steps of prove_step_custom at t = 5:
    the serialised proof is the one from the POW tape's checkpoints, and it verifies"""
    field, t, every, steps = FIELD_FQ, 5, 5, 3
    m = MOD[field]
    z0, ref_cps, last = chain(field, t, steps, every)
    i0 = o.from_mont(int.from_bytes(z0[2], "little"), m)
    per = steps * t // every + 1
    start = np.frombuffer(z0[0] + z0[1], dtype="<u8").reshape(2, 4).copy()
    out = []
    for kind in ("minroot", "pow"):
        xy = np.zeros((per, 8), dtype="<u8")
        ctx.round_tape_eval_batch(field, minroot_tape(field, kind), None, start, 1, steps * t, xy, every=every, j_base=i0)
        cps = np.concatenate([xy, mont_rows([i0 + k * every for k in range(per)], m)], axis=1)
        assert cps.tobytes() == ref_cps.tobytes()
        d_window, ok = window_by_walks(ctx, field, t, steps, every, cps)
        assert ok == [1] * (steps * t // every)
        d_steps = d_window.view(steps, 2 * (t + 1), 4)
        pp, proof = prove(ctx, field, t, [d_steps[g] for g in range(steps)], z0)
        assert proof.verify(pp, steps, list(z0), [last.x, last.y, last.i]) is True
        out.append(proof.serialize())
        proof.free(); pp.free()
    assert out[0] == out[1]


def test_the_c_example_evaluates_chains_by_an_addition_chain(ctx):
    exe = os.path.join(ROOT, "examples", "eval_custom_chain")
    assert os.path.exists(exe), "examples/eval_custom_chain is built by vdf_amd/csrc/Makefile (all)"
    n, rounds = 130, 64
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run([exe, str(n), str(rounds)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["differ from vdf_minroot_eval_batch"] == "0"
    assert lines["chain"].startswith("32 steps, 9 temporaries, 283 products")
    # the Python path over the same chains
    m = o.Q
    start = mont_rows([v for w in range(n) for v in (1000 + w, w)], m)
    out = np.zeros((n, 8), dtype="<u8")
    ctx.round_tape_eval_batch(FIELD_FQ, minroot_tape(FIELD_FQ, "minroot"), None, start, n, rounds, out, j_base=0, j_walk_step=7)
    fnv = 0xcbf29ce484222325
    for b in out.tobytes():
        fnv = ((fnv ^ b) * 0x100000001b3) % 2**64
    assert int(lines["final entries fnv1a64"], 16) == fnv
