"""GPU: a custom delay function evaluated on the device by forward walk tapes (include/vdf_hip.h vdf_round_tape_forward_walk /
vdf_round_tape_eval_batch, kernel k_tape_forward_walk, op VDF_TAPE_POW; include/vdf_nova.h vdf_nova_forward_body_record).

a. the MinRoot forward round recorded as a forward body equals vdf_minroot_forward_walk, landings, trace and checkpoints byte for
   byte: a partial wavefront, a full one, a second and a third workgroup; both fields;
b. a body of every op and six powers on the device equals the host evaluator and a big-integer interpretation;
c. the LDS cap, the layout and the cut walk, as in tests/test_custom_forward_host.py;
d. round_tape_eval_batch equals vdf_minroot_eval_batch, host and device pointers;
e. the work cap: 2^20 products in one launch run, one beyond is refused; the launcher's refusals, after which the context works;
f. end to end with no MinRoot call: circuit F of rounds_spec proved from checkpoints that round_tape_eval_batch made and advice
   that round_tape_walk rebuilt -- the same proof bytes as from vdf_minroot_eval_checkpoints' checkpoints;
g. the plain-C example, as a fresh child process."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import pasta as o
from util import dev, host, mont_states
from rounds_spec import F, MOD, mont_rows
from walks_spec import GUARD, expected_bytes, guarded, minroot_body, start_entries, tape_ints
from forward_tape_spec import (CP_STRIDE, LAYOUT, LAYOUT_FRONT, LAYOUT_TRACE, every_op_forward_body, every_op_forward_ints, layout_cp_entries,
                               layout_expected, minroot_forward_body, model_forward)
from test_gpu_custom_walk import chain, dguard, prove, wide_body, window_by_walks
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError, FORWARD_TAPE_MAX_WORK, WALK_MAX_SLOTS
from vdf_amd.minroot import State
from vdf_amd.nova import WalkBody, forward_tape_eval, record_forward_body, record_walk_body, shape_digest_custom, FIELD_FP, FIELD_FQ

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I0 = 0xFEDCBA


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("rounds", [1, 2, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_a_minroot_forward_tape_equals_the_forward_walk_kernel(ctx, n, rounds, field):
    m, every = MOD[field], {1: 1, 2: 1, 5: 5, 64: 16}[rounds]
    K, stride = rounds // every, rounds + 3
    cps = K + 2                                        # entries nobody writes behind every run of both arrays
    tape = record_forward_body(minroot_forward_body(field), field)
    rng = np.random.default_rng(1000 * n + rounds + field)
    xy = rng.integers(1, 2**62, size=(n, 2))
    # chain w's counter starts at I0 + 1000 w
    rows = [(int(xy[w, 0]) ** 4, int(xy[w, 1]) ** 3, I0 + 1000 * w) for w in range(n)]
    rows[0] = (5, m - 5, I0)                           # x + y = 0: the root of zero
    states = mont_states([[v % m for v in r] for r in rows], m)
    d_states, d_entries = dev(states), dev(np.ascontiguousarray(states[:, :8]))
    want_tr, got_tr = dguard(2 * (n * stride + 1)), dguard(2 * (n * stride + 1))
    want_cp, got_cp = dguard(3 * (n * cps + 1)), dguard(2 * (n * cps + 1))
    ctx.minroot_forward_walk(field, d_states, n, rounds, want_cp, every, cps, want_tr, stride, 0)
    ctx.round_tape_forward_walk(field, tape, None, d_entries, n, rounds, got_cp, every, cps, got_tr, stride, 0, j_base=I0, j_walk_step=1000)
    ctx.sync()
    g, w = host(got_tr), host(want_tr)
    assert g.tobytes() == w.tobytes()
    gt = g.reshape(-1, 8)
    assert int((gt[:, 0] != np.uint64(GUARD)).sum()) == n * rounds   # (a canonical x never has an all-ones limb)
    assert (gt[n * stride:] == np.uint64(GUARD)).all() and (gt[0] == np.uint64(GUARD)).all()
    gc, wc = host(got_cp).reshape(-1, 8), host(want_cp).reshape(-1, 12)
    assert gc.tobytes() == np.ascontiguousarray(wc[:, :8]).tobytes()      # (guards are all-ones on both sides)
    assert int((gc[:, 0] != np.uint64(GUARD)).sum()) == n * K
    assert host(d_entries).reshape(n, 8).tobytes() == np.ascontiguousarray(host(d_states).reshape(n, 12)[:, :8]).tobytes()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("rounds", [1, 2, 5])
def test_a_body_of_every_op_on_the_device(ctx, rounds, field):
    m, n = MOD[field], 65
    tape = record_forward_body(every_op_forward_body(field), field)
    start = start_entries(n, 3, m, np.random.default_rng(field + rounds))
    inv, kw = [m - 1], dict(walk_stride=rounds + 2, j_base=2**64 - 3, j_walk_step=1)
    n_tr = 3 * (n * (rounds + 2) + 1)
    d_entries, d_trace = dev(mont_rows(start, m)), dguard(n_tr)
    ctx.round_tape_forward_walk(field, tape, mont_rows(inv, m), d_entries, n, rounds, trace=d_trace, **kw)
    ctx.sync()
    entries, trace = mont_rows(start, m), guarded(n_tr)
    forward_tape_eval(field, tape, mont_rows(inv, m), entries, n, rounds, trace=trace, **kw)
    assert host(d_entries).tobytes() == entries.tobytes() and host(d_trace).tobytes() == trace.tobytes()
    land, tr = list(start), [None] * n_tr
    model_forward(every_op_forward_ints, m, 3, inv, land, n, rounds, trace=tr, **kw)
    assert tape_ints(entries, m) == land and trace.tobytes() == expected_bytes(tr, m)


def test_the_lds_cap_runs_and_one_beyond_is_refused(ctx):
    """n_slots + 2 n_adv = 32 is 64 KiB of LDS: it launches and is exact; 33 is refused before a launch"""
    field, m, n, rounds, na = FIELD_FQ, o.Q, 65, 3, 5
    tape = record_forward_body(wide_body(WALK_MAX_SLOTS - 2 * na, na), field)
    assert tape.c.n_slots + 2 * na == WALK_MAX_SLOTS
    start = start_entries(n, na, m, np.random.default_rng(9))
    d_entries, entries = dev(mont_rows(start, m)), mont_rows(start, m)
    ctx.round_tape_forward_walk(field, tape, None, d_entries, n, rounds)
    ctx.sync()
    forward_tape_eval(field, tape, None, entries, n, rounds)
    assert host(d_entries).tobytes() == entries.tobytes()
    # s = (x + j) (2^22 - 1): the body's sum of 22 doublings
    land = list(start)
    model_forward(lambda cur, j, inv, mm: [(cur[0] + j) * (2**22 - 1) % mm] * na, m, na, [], land, n, rounds)
    assert tape_ints(entries, m) == land
    tape.c.n_slots += 1
    with pytest.raises(VdfError) as e:
        ctx.round_tape_forward_walk(field, tape, None, d_entries, n, rounds)
    assert e.value.code == VDF_ERR_BAD_ARG
    ctx.sync()
    assert host(d_entries).tobytes() == entries.tobytes()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("every", [1, 2, 5])
def test_strides_base_every_the_counter_and_a_cut_walk(ctx, every, field):
    import torch
    m = MOD[field]
    tape = record_forward_body(every_op_forward_body(field), field)
    start, inv, want_tr, want_cp, land = layout_expected(field, every)
    inv_m, n_cp = mont_rows(inv, m), layout_cp_entries(every)
    d_entries, d_tr, d_cp = dev(mont_rows(start, m)), dguard(3 * LAYOUT_TRACE), dguard(3 * n_cp)
    ctx.round_tape_forward_walk(field, tape, inv_m, d_entries, checkpoints=d_cp[3 * LAYOUT_FRONT:], every=every, cp_stride=CP_STRIDE[every],
                                trace=d_tr[3 * LAYOUT_FRONT:], **LAYOUT)
    d_entries2, d_tr2, d_cp2 = dev(mont_rows(start, m)), dguard(3 * LAYOUT_TRACE), dguard(3 * n_cp)
    cut = dict(LAYOUT)
    for rounds, base in ((3, 3), (2, 6)):
        cut.update(rounds=rounds, base=base)
        ctx.round_tape_forward_walk(field, tape, inv_m, d_entries2, checkpoints=d_cp2[3 * LAYOUT_FRONT:], every=every,
                                    cp_stride=CP_STRIDE[every], trace=d_tr2[3 * LAYOUT_FRONT:], **cut)
    ctx.sync()
    assert tape_ints(host(d_entries), m) == land
    assert host(d_tr).tobytes() == expected_bytes(want_tr, m) and host(d_cp).tobytes() == expected_bytes(want_cp, m)
    assert torch.equal(d_entries, d_entries2) and torch.equal(d_tr, d_tr2) and torch.equal(d_cp, d_cp2)


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_eval_batch_equals_the_minroot_eval_batch(ctx, field):
    m, n, T = MOD[field], 65, 130
    tape = record_forward_body(minroot_forward_body(field), field)
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
    # refusals of the call itself, before anything is enqueued
    out = np.zeros((n, 8), dtype="<u8")
    for bad in (dict(every=7), dict(launch_rounds=FORWARD_TAPE_MAX_WORK)):
        with pytest.raises(VdfError) as e:
            ctx.round_tape_eval_batch(field, tape, None, start, n, T, out, **bad)
        assert e.value.code == VDF_ERR_BAD_ARG
    with pytest.raises(VdfError) as e:
        ctx.round_tape_eval_batch(7, tape, None, start, n, T, out)
    assert e.value.code == VDF_ERR_BAD_ARG
    assert not out.any()
    ctx.round_tape_eval_batch(field, tape, None, start, 0, T, out)             # nothing to do
    ctx.round_tape_eval_batch(field, tape, None, start, n, 0, out)             # no round: the initial entries
    assert out.tobytes() == start.tobytes()


def test_the_work_cap_runs_and_one_beyond_is_refused(ctx):
    """255 squarings and one product per round: 4,096 rounds are exactly VDF_FORWARD_TAPE_MAX_WORK = 2^20 products in one launch"""
    field, m = FIELD_FQ, o.Q
    tape = record_forward_body(WalkBody(0, 1, lambda c, j, inv, cur: [c.mul(c.pow(cur[0], 2**255), cur[0])]), field)
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


def test_the_launcher_refuses_and_the_context_goes_on(ctx):
    field, m = FIELD_FQ, o.Q
    fresh = lambda: record_forward_body(every_op_forward_body(field), field)
    inv = mont_rows([5], m)
    start = mont_rows(list(range(1, 13)), m)
    d_entries, d_trace, d_cp = dev(start), dguard(3 * 30), dguard(3 * 30)
    good = dict(trace=d_trace, walk_stride=7, checkpoints=d_cp, every=2, cp_stride=7)

    def refused(tape=None, entries=d_entries, rounds=5, field=field, inv=inv, **kw):
        args = dict(good)
        args.update(kw)
        with pytest.raises(VdfError) as e:
            ctx.round_tape_forward_walk(field, tape or fresh(), inv, entries, 4, rounds, **args)
        assert e.value.code == VDF_ERR_BAD_ARG
    h = np.zeros((3 * 30, 4), dtype="<u8")
    refused(entries=start.copy())                      # a host pointer for entries / trace / checkpoints
    refused(trace=h)
    refused(checkpoints=h)
    refused(inv=dev(inv))                              # a device pointer for inv
    refused(every=0)                                   # checkpoints without every
    refused(field=7)
    t = fresh()
    ops = t.op_list()
    t.ops[next(i for i, x in enumerate(ops) if x[0] == 0)].b = 1
    refused(tape=t)                                    # ADV of the entry being produced
    t = fresh()
    t.ops[next(i for i, x in enumerate(ops) if x[0] == 9)].b = 8
    refused(tape=t)                                    # the exponent of a POW: a constant the tape does not have
    t = fresh()
    t.c.n_vars = 2
    refused(tape=t)                                    # n_vars != n_adv
    # a POW in a round tape and in a descending walk tape
    w = record_walk_body(minroot_body(field), field)
    ctx.round_tape_walk(field, w, inv, dev(start), 4, 1)
    w.ops[next(i for i, x in enumerate(w.op_list()) if x[0] == 6)].op = 9
    w.ops[next(i for i, x in enumerate(w.op_list()) if x[0] == 9)].b = 0
    w.c.n_consts = 1
    with pytest.raises(VdfError) as e:
        ctx.round_tape_walk(field, w, inv, d_entries, 4, 1)
    assert e.value.code == VDF_ERR_BAD_ARG
    p = record_forward_body(WalkBody(0, 1, lambda c, j, inv, cur: [c.pow(cur[0], 5)]), field)
    with pytest.raises(VdfError) as e:
        ctx.round_tape_run(field, p, 4, None, d_entries, d_trace)
    assert e.value.code == VDF_ERR_BAD_ARG
    ctx.sync()
    assert host(d_entries).tobytes() == start.tobytes() and (host(d_trace) == np.uint64(GUARD)).all() and (host(d_cp) == np.uint64(GUARD)).all()
    # the next valid call on the same context succeeds
    ctx.round_tape_forward_walk(field, fresh(), inv, d_entries, 4, 5, **good)
    ctx.sync()
    want, tr, cp = start.copy(), guarded(3 * 30), guarded(3 * 30)
    forward_tape_eval(field, fresh(), inv, want, 4, 5, cp, 2, 7, tr, 7)
    assert host(d_entries).tobytes() == want.tobytes() and host(d_trace).tobytes() == tr.tobytes() and host(d_cp).tobytes() == cp.tobytes()
    ctx.round_tape_forward_walk(field, fresh(), inv, d_entries, 0, 5)      # nothing to do
    ctx.round_tape_forward_walk(field, fresh(), inv, d_entries, 4, 0)
    ctx.sync()
    assert host(d_entries).tobytes() == want.tobytes()


# ---- end to end with no MinRoot call: circuit F proved from checkpoints the forward tape made ------------------------------------
def checkpoints_by_the_forward_tape(ctx, field, t, steps, every, z0):
    """uint64[steps * t / every + 1, 12]: (x, y) by round_tape_eval_batch, the counter column stated (window_by_walks reads row 0's)"""
    m = MOD[field]
    i0 = o.from_mont(int.from_bytes(z0[2], "little"), m)
    per = steps * t // every + 1
    tape = record_forward_body(minroot_forward_body(field), field)
    start = np.frombuffer(z0[0] + z0[1], dtype="<u8").reshape(2, 4).copy()
    out = np.zeros((per, 8), dtype="<u8")
    ctx.round_tape_eval_batch(field, tape, None, start, 1, steps * t, out, every=every, j_base=i0)
    return np.concatenate([out, mont_rows([i0 + k * every for k in range(per)], m)], axis=1)


def pipeline(ctx, field, t, every, steps=3):
    z0, ref_cps, last = chain(field, t, steps, every)          # vdf_minroot_eval_checkpoints: the reference only
    cps = checkpoints_by_the_forward_tape(ctx, field, t, steps, every, z0)
    assert cps.tobytes() == ref_cps.tobytes()
    zi = [cps[-1, 0:4].tobytes(), cps[-1, 4:8].tobytes(), cps[-1, 8:12].tobytes()]
    assert zi == [last.x, last.y, last.i]
    out = []
    for c in (cps, ref_cps):
        d_window, ok = window_by_walks(ctx, field, t, steps, every, c)
        assert ok == [1] * (steps * t // every)
        d_steps = d_window.view(steps, 2 * (t + 1), 4)
        pp, proof = prove(ctx, field, t, [d_steps[g] for g in range(steps)], z0)
        assert proof.verify(pp, steps, list(z0), zi) is True
        snark = proof.compress(pp)
        assert snark.verify(pp, steps, list(z0), zi) is True
        out.append((proof.serialize(), snark.serialize()))
        proof.free(); pp.free()
    assert out[0] == out[1]


def test_the_whole_pipeline_one_walk_per_step(ctx):
    pipeline(ctx, FIELD_FQ, 5, 5)


def test_the_whole_pipeline_five_walks_per_step(ctx):
    pipeline(ctx, FIELD_FQ, 65, 13)


def test_the_whole_pipeline_in_the_other_orientation(ctx):
    pipeline(ctx, FIELD_FP, 5, 5)


def test_the_c_example_runs_the_whole_pipeline(ctx):
    exe = os.path.join(ROOT, "examples", "prove_custom_pipeline")
    assert os.path.exists(exe), "examples/prove_custom_pipeline is built by vdf_amd/csrc/Makefile (all)"
    src = open(exe + ".c").read()
    assert "vdf_minroot_" not in src                  # the example evaluates its chain through the seam alone
    t, every, steps, x0 = 65, 13, 3, 123
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run([exe, str(t), str(every), str(steps), str(x0)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["walks ok"] == "%d of %d" % (steps * t // every, steps * t // every)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true"
    assert int(lines["digest"], 16) == shape_digest_custom(F(t, "repeat"))[0]
    # the Python path at the same t and steps, through the same three tapes
    s0 = State.from_ints(FIELD_FQ, x0, 0, 0)
    z0 = (s0.x, s0.y, s0.i)
    cps = checkpoints_by_the_forward_tape(ctx, FIELD_FQ, t, steps, every, z0)
    d_window, ok = window_by_walks(ctx, FIELD_FQ, t, steps, every, cps)
    assert ok == [1] * (steps * t // every)
    d_steps = d_window.view(steps, 2 * (t + 1), 4)
    pp, proof = prove(ctx, FIELD_FQ, t, [d_steps[g] for g in range(steps)], z0)
    snark = proof.compress(pp)
    assert lines["compressed proof sha256"] == hashlib.sha256(snark.serialize()).hexdigest()
    proof.free(); pp.free()
