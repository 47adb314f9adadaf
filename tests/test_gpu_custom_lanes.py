"""GPU: custom chains in lanes (include/vdf_hip.h vdf_round_tape_run_lanes / kernel k_round_tape_lanes, vdf_round_tape_walk_lanes /
kernel k_tape_walk_lanes; include/vdf_nova.h vdf_cs_repeat_lanes, vdf_nova_custom_chain_lanes_from_checkpoints).

a. k_round_tape_lanes writes byte for byte what `lanes` calls of vdf_round_tape_run write, and the host evaluator's bytes: partial
   wavefronts, a full one, several workgroups, 1 to 16 lanes, both fields, lane_stride = t + 1 and t + 4; guard elements behind
   the variables (and between the lanes of the separate calls) stay untouched;
b. k_tape_walk_lanes: entries, trace and ok byte for byte the host restatement's AND those of `lanes` separate vdf_round_tape_walk
   calls; lanes and steps cross a wavefront boundary, the walks are cut into launches of 4 rounds, three columns, per-lane inv all
   distinct, one lane's counter wraps; a corrupted checkpoint of lane 3 of step 1 clears exactly that ok;
c. proofs made four ways -- repeat_lanes with device advice, with host advice, the plain double loop, and prove_recursively_custom
   over a lanes chain -- have the same running and compressed bytes and verify; over Fp; with periodic_rows = 1 (the generic kernel);
   one lane is today's cs.repeat proof; a wrong advice entry in lane 1 is verify = False, and under check_steps an error naming
   step, lane, repetition and constraint; a chain whose lanes are not the parameters' is refused;
d. chains 2 .. 4 of a vdf_round_tape_eval_batch DEVICE array as a lanes chain: the proof over the host copy of the same checkpoints;
e. the plain-C example, as a fresh child process."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from custom_chain_spec import I0, X0, forward_minroot_body, step_traces, z0_of
from custom_lanes_spec import (FL, every_op_lanes_chain, lanes_checkpoints, lane_start, step_advice_ints, walk_at_the_slot_cap,
                               walk_inv_and_j_base, window_walks, z_of)
from rounds_spec import F, G, MOD, mont_rows
from util import dev, dev_read, host
from walks_spec import GUARD, every_op_body, guarded, minroot_body
from vdf_amd._lib import VDF_ERR_BAD_ARG, lib
from vdf_amd.hip import VdfError
from vdf_amd.nova import (CustomChain, NovaVDFProof, custom_chain_slices, public_params_custom, record_forward_body, record_round_body,
                          record_walk_body, round_tape_eval_lanes, shape_digest_custom, walk_tape_eval_lanes, FIELD_FP, FIELD_FQ)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
_PP = {}


@pytest.fixture(scope="module", autouse=True)
def free_the_parameter_sets():
    yield
    for pp in _PP.values():
        pp.free()
    _PP.clear()


def params(ctx, field, lanes, t, mode="repeat", periodic=0):
    """one parameter set per shape for the whole module"""
    key = (field, lanes, t, mode, periodic)
    if key not in _PP:
        _PP[key] = public_params_custom(ctx, FL(t, lanes, mode, field), field=field, periodic_rows=periodic)
    return _PP[key]


def dguard(n_elems):
    import torch
    g = torch.full((n_elems, 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                           # (the fill runs on torch's stream, the library's kernels on the context's)
    return g


# ---- a. k_round_tape_lanes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("gap", [0, 3])
@pytest.mark.parametrize("lanes,t", [(1, 65), (2, 63), (3, 64), (16, 65), (5, 257)])
def test_the_rounds_of_all_lanes_in_one_launch(ctx, lanes, t, gap, field):
    m, stride, nv = MOD[field], t + 1 + gap, 5
    tape = record_round_body(G(t, "repeat", field).body(), field)
    rng = np.random.default_rng(1000 * lanes + t + gap + field)
    adv = rng.integers(0, 2**62, size=3 * ((lanes - 1) * stride + t + 1)).tolist()
    adv[1], adv[4], adv[7] = 0, 1, m - 1
    inv = [(0xABCDEF + 17 * l) ** 3 % m for l in range(lanes)]
    adv_m, inv_m = mont_rows(adv, m), mont_rows(inv, m)
    d_adv, d_out = dev(adv_m), dguard(lanes * t * nv + 2)
    ctx.round_tape_run_lanes(field, tape, t, lanes, inv_m, d_adv, stride, d_out)
    # ... and lane after lane by the single call, a guard element between the lanes
    d_sep = dguard(lanes * (t * nv + 1))
    for l in range(lanes):
        ctx.round_tape_run(field, tape, t, inv_m[l:l + 1].copy(), d_adv[3 * l * stride:], d_sep[l * (t * nv + 1):])
    ctx.sync()
    got, sep = host(d_out), host(d_sep).reshape(lanes, t * nv + 1, 4)
    assert (got[lanes * t * nv:] == np.uint64(GUARD)).all() and (sep[:, -1] == np.uint64(GUARD)).all()
    assert got[:lanes * t * nv].tobytes() == np.ascontiguousarray(sep[:, :-1]).tobytes()
    assert got[:lanes * t * nv].tobytes() == round_tape_eval_lanes(field, tape, t, lanes, inv_m, adv_m, stride).tobytes()
    assert host(d_adv).tobytes() == adv_m.tobytes()


def test_the_launcher_of_the_rounds_refuses_and_the_context_goes_on(ctx):
    field, m, t = FIELD_FQ, MOD[FIELD_FQ], 5
    tape = record_round_body(G(t, "repeat", field).body(), field)
    inv_m = mont_rows(list(range(1, 20)), m)
    d_adv, d_out = dev(mont_rows(list(range(1, 3 * 17 * (t + 1) + 1)), m)), dguard(17 * t * 5)

    def refused(lanes, stride=t + 1, advice=d_adv, out=d_out):
        with pytest.raises(VdfError) as e:
            ctx.round_tape_run_lanes(field, tape, t, lanes, inv_m, advice, stride, out)
        assert e.value.code == VDF_ERR_BAD_ARG
    refused(0)
    refused(17)
    refused(2, stride=t)
    refused(2, advice=mont_rows([1] * (6 * (t + 1)), m))          # a host pointer
    ctx.sync()
    assert (host(d_out) == np.uint64(GUARD)).all()
    ctx.round_tape_run_lanes(field, tape, t, 16, inv_m, d_adv, t + 1, d_out)
    ctx.sync()
    assert host(d_out)[:16 * t * 5].tobytes() == round_tape_eval_lanes(field, tape, t, 16, inv_m, host(d_adv), t + 1).tobytes()
    assert (host(d_out)[16 * t * 5:] == np.uint64(GUARD)).all()


# ---- b. k_tape_walk_lanes ----------------------------------------------------------------------------------------------------------
def walk_window(ctx, field, steps, lanes, t, every, launch_rounds, corrupt=None):
    """the window on the device by vdf_round_tape_walk_lanes (cut into launches), on the host (one uncut call), and by `lanes`
    separate vdf_round_tape_walk calls over the same trace layout; corrupt = (step, lane, walk): that checkpoint is wrong"""
    import torch
    m, per = MOD[field], t // every
    tape = record_walk_body(every_op_body(field), field)
    inv, j_base, cps = every_op_lanes_chain(field, t, steps, every, lanes)
    assert len(set(inv)) == lanes and (lanes == 1 or j_base[1] == 2**64 - 12)
    starts, expect = window_walks(cps, lanes, per, 0, steps)
    n, n_tr = steps * lanes * per, 3 * (steps * lanes * (t + 1) + 1)
    want_ok = [1] * n
    if corrupt:
        w = (corrupt[0] * lanes + corrupt[1]) * per + corrupt[2]
        expect = list(expect)
        expect[3 * w + 1] ^= 1
        want_ok[w] = 0
    inv_m, starts_m, expect_m = mont_rows(inv, m), mont_rows(starts, m), mont_rows(expect, m)
    kw = dict(walk_stride=every, group=per, group_stride=t + 1, j_group_step=t)
    # the host restatement, uncut
    h_entries, h_trace, h_ok = starts_m.copy(), guarded(n_tr), np.full(n + 1, -7, dtype="<i4")
    walk_tape_eval_lanes(field, tape, lanes, inv_m, h_entries, n, every, h_trace, top=every, j_base=j_base, heads=True, expect=expect_m, ok=h_ok, **kw)
    assert h_ok.tolist() == want_ok + [-7]
    # the device, all lanes per launch
    d_entries, d_trace, d_expect = dev(starts_m), dguard(n_tr), dev(expect_m)
    d_ok = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    for rounds, top, last in custom_chain_slices(every, launch_rounds):
        ctx.round_tape_walk_lanes(field, tape, lanes, inv_m, d_entries, n, rounds, d_trace, top=top, j_base=j_base, heads=last,
                                  expect=d_expect if last else None, ok=d_ok if last else None, **kw)
    ctx.sync()
    assert host(d_entries).tobytes() == h_entries.tobytes()
    assert host(d_trace).tobytes() == h_trace.tobytes()
    assert d_ok.cpu().tolist() == h_ok.tolist()
    # lane after lane by the single call: the lane's walks gathered, the trace moved by l (t + 1) entries, groups lanes (t + 1) apart
    s_trace = dguard(n_tr)
    s_entries, s_ok = np.zeros((n, 12), dtype="<u8"), np.zeros(n + 1, dtype="<i4")
    s_ok[n] = -7
    for l in range(lanes):
        mine = [w for w in range(n) if (w // per) % lanes == l]
        dl, xl = dev(starts_m.reshape(n, 12)[mine].reshape(-1, 4)), dev(expect_m.reshape(n, 12)[mine].reshape(-1, 4))
        okl = torch.full((len(mine),), -7, dtype=torch.int32, device="cuda")
        for rounds, top, last in custom_chain_slices(every, launch_rounds):
            ctx.round_tape_walk(field, tape, inv_m[l:l + 1].copy(), dl, len(mine), rounds, s_trace[3 * l * (t + 1):], walk_stride=every, top=top,
                                group=per, group_stride=lanes * (t + 1), j_base=j_base[l], j_group_step=t, heads=last,
                                expect=xl if last else None, ok=okl if last else None)
        ctx.sync()
        s_entries[mine] = host(dl).reshape(-1, 12)
        s_ok[mine] = okl.cpu().numpy()
    assert s_entries.tobytes() == h_entries.tobytes() and host(s_trace).tobytes() == h_trace.tobytes() and s_ok.tolist() == h_ok.tolist()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_walks_of_three_steps_of_five_lanes_cut_into_launches_of_four_rounds(ctx, field):
    """75 walks: lanes and steps cross the boundary between the two wavefronts"""
    walk_window(ctx, field, 3, 5, 65, 13, 4)


@pytest.mark.parametrize("steps,lanes,every", [(1, 16, 65), (2, 2, 1)])
def test_walks_of_sixteen_lanes_and_of_one_round(ctx, steps, lanes, every):
    walk_window(ctx, FIELD_FQ, steps, lanes, 65, every, 0)


def test_one_lane_is_the_single_walk(ctx):
    walk_window(ctx, FIELD_FQ, 2, 1, 65, 13, 4)


def test_a_corrupted_checkpoint_of_lane_three_of_step_one_clears_exactly_that_ok(ctx):
    walk_window(ctx, FIELD_FQ, 3, 5, 65, 13, 4, corrupt=(1, 3, 2))


def test_the_launcher_of_the_walks_refuses_and_the_context_goes_on(ctx):
    field, m = FIELD_FQ, MOD[FIELD_FQ]
    tape = record_walk_body(every_op_body(field), field)
    inv_m, start = mont_rows(list(range(5, 40)), m), mont_rows(list(range(1, 13)), m)
    d_entries, d_trace = dev(start), dguard(3 * 30)

    def refused(lanes, **kw):
        args = dict(trace=d_trace, walk_stride=6, top=5, group=1, group_stride=6)
        args.update(kw)
        with pytest.raises(VdfError) as e:
            ctx.round_tape_walk_lanes(field, tape, lanes, inv_m, d_entries, 4, 5, **args)
        assert e.value.code == VDF_ERR_BAD_ARG
    refused(0)
    refused(17)
    refused(2, top=3)
    refused(2, trace=guarded(3 * 30))
    ctx.sync()
    assert host(d_entries).tobytes() == start.tobytes() and (host(d_trace) == np.uint64(GUARD)).all()
    ctx.round_tape_walk_lanes(field, tape, 4, inv_m, d_entries, 4, 5, d_trace, walk_stride=6, top=5, group=1, group_stride=6, j_base=[1, 2, 3, 4])
    ctx.sync()
    want, tr = start.copy(), guarded(3 * 30)
    walk_tape_eval_lanes(field, tape, 4, inv_m, want, 4, 5, tr, walk_stride=6, top=5, group=1, group_stride=6, j_base=[1, 2, 3, 4])
    assert host(d_entries).tobytes() == want.tobytes() and host(d_trace).tobytes() == tr.tobytes()


def test_the_lds_cap_in_lanes_runs_and_one_beyond_is_refused(ctx):
    """n_slots + 2 n_adv + n_inv = 32 is 64 KiB of LDS: it launches and is exact; 33 is refused before a launch"""
    field, m, n, rounds, na, lanes = FIELD_FQ, MOD[FIELD_FQ], 65, 3, 5, 3
    tape = walk_at_the_slot_cap(na, 2)
    inv_m = mont_rows(list(range(3, 3 + 2 * lanes)), m)
    start = mont_rows(np.random.default_rng(9).integers(0, 2**62, size=n * na).tolist(), m)
    d_entries, entries = dev(start), start.copy()
    kw = dict(group=4, j_base=[7, 2**64 - 2, 9], j_group_step=5)
    ctx.round_tape_walk_lanes(field, tape, lanes, inv_m, d_entries, n, rounds, **kw)
    ctx.sync()
    walk_tape_eval_lanes(field, tape, lanes, inv_m, entries, n, rounds, **kw)
    assert host(d_entries).tobytes() == entries.tobytes() != start.tobytes()
    tape.c.n_slots += 1
    with pytest.raises(VdfError) as e:
        ctx.round_tape_walk_lanes(field, tape, lanes, inv_m, d_entries, n, rounds, **kw)
    assert e.value.code == VDF_ERR_BAD_ARG
    ctx.sync()
    assert host(d_entries).tobytes() == entries.tobytes()


# ---- c. proofs -------------------------------------------------------------------------------------------------------------------
def proof_bytes(pp, proof):
    snark = proof.compress(pp)
    out = proof.serialize(), snark.serialize()
    snark.free(); proof.free()
    return out


def by_steps(ctx, field, lanes, t, mode, device=False, base=(X0, I0), periodic=0, stride=None):
    """vdf_nova_prove_step_custom step by step over the steps' advice; verified; (running bytes, compressed bytes)"""
    pp, c, proof = params(ctx, field, lanes, t, "loop" if mode == "loop" else "repeat", periodic), FL(t, lanes, mode, field, stride), None
    m, keep = MOD[field], []
    for g in range(STEPS):
        ints = step_advice_ints(field, t, STEPS, lanes, g, stride, base)
        c.advice_ints = ints
        c.advice = dev(mont_rows(ints, m)) if device else mont_rows(ints, m)
        keep.append(c.advice)
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z_of(field, lanes, base=base))
    ctx.sync()
    assert proof.verify(pp, STEPS, z_of(field, lanes, base=base), z_of(field, lanes, t, STEPS, base)) is True
    snark = proof.compress(pp)
    assert snark.verify(pp, STEPS, z_of(field, lanes, base=base), z_of(field, lanes, t, STEPS, base)) is True
    out = proof.serialize(), snark.serialize()
    snark.free(); proof.free()
    return out


def lanes_chain(field, lanes, t, every, cps=None, stride=None, base=(X0, I0)):
    inv, j_base = walk_inv_and_j_base(field, lanes, base)
    if cps is None:
        cps = lanes_checkpoints(field, t, STEPS, every, lanes, stride, base)
    return CustomChain.lanes_from_checkpoints(field, record_walk_body(minroot_body(field), field), inv, t, every, STEPS, lanes, cps, stride, j_base)


def by_chain(ctx, field, lanes, t, every, window_steps, periodic=0, **kw):
    pp, chain = params(ctx, field, lanes, t, periodic=periodic), lanes_chain(field, lanes, t, every, **kw)
    proof = NovaVDFProof.prove_recursively_custom(pp, FL(t, lanes, "repeat", field), chain, z_of(field, lanes, base=kw.get("base", (X0, I0))),
                                                  window_steps=window_steps, check_steps=True)
    assert proof.num_steps() == STEPS and chain.memory() == (0, 0)
    chain.free()
    return proof_bytes(pp, proof)


@pytest.mark.parametrize("lanes,t,every", [(2, 5, 5), (3, 65, 13)])
def test_four_ways_to_the_same_proof(ctx, lanes, t, every):
    field = FIELD_FQ
    pp = params(ctx, field, lanes, t)
    assert pp.repeat_lanes() == lanes and pp.repeat_rows()[2] == t and pp.segment()[1] == lanes * t * 3
    assert pp.digest() == params(ctx, field, lanes, t, "loop").digest() == shape_digest_custom(FL(t, lanes))[0]
    want = by_steps(ctx, field, lanes, t, "repeat", device=True)
    assert by_steps(ctx, field, lanes, t, "repeat") == want
    assert by_steps(ctx, field, lanes, t, "loop") == want
    assert by_chain(ctx, field, lanes, t, every, 2) == want
    assert by_chain(ctx, field, lanes, t, every, 0) == want
    # a wider stride of the advice, host and device, is the same proof
    assert by_steps(ctx, field, lanes, t, "repeat", device=True, stride=t + 4) == want


def test_the_other_orientation(ctx):
    field, lanes, t = FIELD_FP, 2, 5
    want = by_steps(ctx, field, lanes, t, "repeat", device=True)
    assert by_steps(ctx, field, lanes, t, "repeat") == want == by_steps(ctx, field, lanes, t, "loop")
    assert by_chain(ctx, field, lanes, t, 5, 2) == want


def test_periodic_rows_of_lanes_keep_the_generic_kernel(ctx):
    field, lanes, t = FIELD_FQ, 2, 5
    pp = params(ctx, field, lanes, t, periodic=1)
    assert pp.periodic_rows() is None and pp.stencil() != 7
    assert params(ctx, field, 1, t, periodic=1).stencil() == 7         # one lane: the rows are periodic and run from their description
    want = by_steps(ctx, field, lanes, t, "repeat", device=True)
    assert by_steps(ctx, field, lanes, t, "repeat", device=True, periodic=1) == want
    assert by_chain(ctx, field, lanes, t, 5, 2, periodic=1) == want


def test_one_lane_is_the_proof_of_the_single_repeat(ctx):
    field, t = FIELD_FQ, 5
    want = by_steps(ctx, field, 1, t, "repeat", device=True)
    assert by_chain(ctx, field, 1, t, 5, 2) == want
    pp, c, proof = public_params_custom(ctx, F(t, "repeat", field), field=field), F(t, "repeat", field), None
    assert pp.repeat_lanes() == 1
    for tr in step_traces(field, t, STEPS):
        c.advice = dev(tr)
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0_of(field))
    ctx.sync()
    assert proof_bytes(pp, proof) == want
    pp.free()


def test_a_wrong_advice_entry_in_lane_one(ctx):
    field, lanes, t, every, m = FIELD_FQ, 3, 65, 13, MOD[FIELD_FQ]
    pp, z0, zi = params(ctx, field, lanes, t), z_of(field, lanes), z_of(field, lanes, t, STEPS)
    # entry 7 of lane 1 in step 1, through device advice and through host advice
    for device in (True, False):
        c, proof, keep = FL(t, lanes, "repeat", field), None, []
        for g in range(STEPS):
            adv = mont_rows(step_advice_ints(field, t, STEPS, lanes, g), m)
            if g == 1:
                adv[2 * (1 * (t + 1) + 7), 0] ^= np.uint64(1)
            c.advice = dev(adv) if device else adv
            keep.append(c.advice)
            proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
        ctx.sync()
        assert proof.verify(pp, STEPS, z0, zi) is False
        proof.free()
    # the same entry of a chain's resident trace: every walk has landed, the step's rows disagree
    chain = lanes_chain(field, lanes, t, every)
    assert chain.materialize(ctx, 0, STEPS) == [0] * STEPS
    at = chain.advice(1) + 2 * (1 * (t + 1) + 7) * 32
    x = dev_read(ctx, at, 32)
    x[0] ^= np.uint64(1)
    assert lib.vdf_dev_memcpy(ctx.handle, at, x.ctypes.data, 32) == 0
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, FL(t, lanes, "repeat", field), chain, z0, window_steps=4, check_steps=True)
    msg = str(e.value)
    # x_7 is the root repetition 6 allocates: its products are made from it, x_7^5 = x_6 + y_6 (constraint 2) fails
    assert e.value.code == VDF_ERR_BAD_ARG and "step 1:" in msg and "lane 1, repetition 6, constraint 2 of the repeat" in msg, msg
    rb, nc, rt = pp.repeat_rows()
    assert "first row %d " % (rb + (1 * t + 6) * nc + 2) in msg, msg
    chain.free()
    # a missed walk names its step and lane
    cps = lanes_checkpoints(field, t, STEPS, every, lanes)
    per_lane = STEPS * (t // every) + 1
    cps[2 * (2 * per_lane + 1 * (t // every) + 2), 0] ^= np.uint64(1)          # lane 2, a middle checkpoint of step 1
    chain = lanes_chain(field, lanes, t, every, cps=cps)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, FL(t, lanes, "repeat", field), chain, z0, window_steps=2)
    assert e.value.code == VDF_ERR_BAD_ARG and "step 1, lane 2: a walk did not land" in str(e.value), str(e.value)
    assert chain.memory() == (0, 0)
    chain.free()
    # ... and the next call with the same parameters is the good proof
    assert by_chain(ctx, field, lanes, t, every, 2) == by_steps(ctx, field, lanes, t, "repeat")


def test_a_chain_whose_lanes_are_not_the_parameters_is_refused(ctx):
    field, t = FIELD_FQ, 5
    pp = params(ctx, field, 2, t)
    for lanes in (1, 3):
        chain = lanes_chain(field, lanes, t, 5)
        with pytest.raises(VdfError) as e:
            NovaVDFProof.prove_recursively_custom(pp, FL(t, 2, "repeat", field), chain, z_of(field, 2), window_steps=2)
        assert e.value.code == VDF_ERR_BAD_ARG and "lanes" in str(e.value), str(e.value)
        chain.free()
    assert by_chain(ctx, field, 2, t, 5, 2) == by_steps(ctx, field, 2, t, "repeat")


def test_a_repeat_that_would_read_past_the_chains_trace_is_refused(ctx):
    """a chain's step trace is lanes * (t + 1) entries: over it the repeat's lane_stride is t + 1.  The stride of the chain's
    CHECKPOINTS (steps * t / every + 1 entries, here 16 with every = 1) is another one, and handing it to the repeat would read
    lanes 1 .. L - 1 behind the trace"""
    field, lanes, t = FIELD_FQ, 2, 5
    pp, z0 = params(ctx, field, lanes, t), z_of(field, lanes)
    want = by_steps(ctx, field, lanes, t, "repeat")
    for stride in (STEPS * t + 1, t + 2):
        chain = lanes_chain(field, lanes, t, 1)
        with pytest.raises(VdfError) as e:
            NovaVDFProof.prove_recursively_custom(pp, FL(t, lanes, "repeat", field, stride), chain, z0, window_steps=2)
        assert e.value.code == VDF_ERR_BAD_ARG and chain.memory() == (0, 0)
        chain.free()
    # step by step: after the refused step the same chain and context go on with the right circuit
    chain = lanes_chain(field, lanes, t, 1)
    chain.materialize(ctx, 0, STEPS)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_step_custom_chain(pp, None, FL(t, lanes, "repeat", field, t + 2), chain, 0, z0)
    assert e.value.code == VDF_ERR_BAD_ARG
    good, proof = FL(t, lanes, "repeat", field), None
    for k in range(STEPS):
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, good, chain, k, z0)
    chain.free()
    assert proof_bytes(pp, proof) == want
    # a wider stride stays legal over a buffer of the caller's own (test_four_ways_to_the_same_proof)


# ---- d. from the evaluator ---------------------------------------------------------------------------------------------------------
def test_chains_two_to_four_of_the_evaluators_device_array(ctx):
    import torch
    field, m, lanes, t, every, n = FIELD_FQ, MOD[FIELD_FQ], 3, 65, 13, 5
    per_lane = STEPS * (t // every) + 1
    fwd = record_forward_body(forward_minroot_body(field), field)
    initial = mont_rows([v for w in range(n) for v in (lane_start(w)[0], 0)], m)
    d_out = torch.zeros((n * per_lane * 2, 4), dtype=torch.int64, device="cuda")
    # chain w counts from I0 + 1000 w: inv = (I0), the counter 1000 per chain apart
    ctx.round_tape_eval_batch(field, fwd, mont_rows([I0], m), initial, n, STEPS * t, d_out, every=every, j_walk_step=1000)
    ctx.sync()
    base = lane_start(2)
    h_out = host(d_out)
    assert h_out[2 * per_lane * 2:].tobytes() == lanes_checkpoints(field, t, STEPS, every, lanes, base=base).tobytes()
    want = by_chain(ctx, field, lanes, t, every, 2, cps=h_out[2 * per_lane * 2:].copy(), base=base)
    got = by_chain(ctx, field, lanes, t, every, 2, cps=d_out.data_ptr() + 2 * per_lane * 2 * 32, stride=per_lane, base=base)
    assert got == want == by_steps(ctx, field, lanes, t, "repeat", base=base)


# ---- e. the C example --------------------------------------------------------------------------------------------------------------
def test_the_c_example_proves_chains_in_lanes(ctx):
    exe = os.path.join(ROOT, "examples", "prove_custom_lanes")
    assert os.path.exists(exe), "examples/prove_custom_lanes is built by vdf_amd/csrc/Makefile (all)"
    t, every, lanes, x0 = 65, 13, 3, 123
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(t), str(every), str(STEPS), str(lanes), str(x0)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true" and lines["lanes of the repeat"] == str(lanes)
    assert lines["resident after the proof"] == "0 steps, 0 bytes"
    assert int(lines["digest"], 16) == shape_digest_custom(FL(t, lanes))[0] == params(ctx, FIELD_FQ, lanes, t).digest()
    # the example proves chains L .. 2 L - 1 of its 2 L: chain w starts at (x0 + w, 0) under the counter 1000 w
    base = (x0 + lanes, 1000 * lanes)
    assert lines["compressed proof sha256"] == hashlib.sha256(by_chain(ctx, FIELD_FQ, lanes, t, every, 2, base=base)[1]).hexdigest()
