"""GPU: the one device interpreter of round tapes (vdf_amd/csrc/rounds.hip tape_round) under each of the six kernels that call it,
and the one statement of the tape rules (vdf_amd/csrc/tape_rules.h) as libvdf_hip.so's launchers apply it.

a. every kernel once, byte for byte against the host evaluator: bodies of every base op with two invariants, 65 repetitions or
   walks (two workgroups, the second with one live lane) and 3 rounds (an odd count: the two entries in LDS end swapped) --
   k_round_tape; k_round_tape_lanes, 3 lanes; k_tape_walk with trace, heads and expect; k_tape_walk_lanes, 3 lanes with their own
   j_base and invariants; k_tape_forward_walk with a POW whose exponent spans two 32-bit words and checkpoints every 2 rounds from
   base 1; k_tape_forward_walk_chain with a POW and a POWC of three temporaries in one tape.
b. the table of tests/tape_rules_spec.py through vdf_round_tape_run, vdf_round_tape_walk and vdf_round_tape_forward_walk: every
   tape is refused with VDF_ERR_BAD_ARG before a launch -- no kernel is timed, nothing is written -- as test_tape_rules_host.py
   sees the host evaluators refuse it."""
import numpy as np
import pytest

from pow_chain_spec import tmp_chain
from rounds_spec import MOD, fe, mont_rows
from tape_rules_spec import FORWARD, N_ADV, ROUND, SENTINEL, WALK, base_tape, cases
from util import dev, host
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.nova import (RoundBody, WalkBody, forward_tape_eval, record_forward_body, record_round_body, record_walk_body, round_tape_eval,
                          round_tape_eval_lanes, walk_tape_eval, walk_tape_eval_lanes, FIELD_FP, FIELD_FQ)

pytestmark = pytest.mark.gpu
N, ROUNDS, LANES = 65, 3, 3


def guard(n_elems):
    return np.full((n_elems, 4), SENTINEL, dtype="<u8")


def elements(rng, n, m):
    vals = [0, 1, m - 1] + [int(rng.integers(1, 2**62)) ** 4 % m for _ in range(n)]
    return mont_rows(vals[:n], m)


def arithmetic(cs, j, inv, a, b, m):
    """every base op of value arithmetic over two advice columns and two invariants: (d, e, h)"""
    d = cs.sub(cs.add(a, b), inv[0])
    e = cs.mul(d, inv[1])
    g = cs.scale(cs.mul(e, e), fe(7, m))
    return d, e, cs.add(cs.add(g, cs.const(fe(11, m))), j)


def round_body(field):
    m = MOD[field]

    def b(cs, j, inv, carry, cur, nxt):
        u = cs.alloc_from(cur[1])
        w = cs.alloc_from(cs.scale(cs.sub(nxt[0], cur[0]), fe(3, m)))
        s = cs.add(cs.sub(cs.mul(u, w), cs.scale(carry[0], fe(7, m))), cs.add(j, cs.const(fe(11, m))))
        return [cs.add(cs.mul(cs.mul(s, inv[0]), inv[1]), u)]
    return RoundBody(2, 1, 2, b)


def walk_body(field):
    return WalkBody(2, 2, lambda cs, j, inv, nxt: [arithmetic(cs, j, inv, nxt[0], nxt[1], MOD[field])[2], nxt[0]])


def forward_body(field, chain):
    def b(cs, j, inv, cur):
        d, e, h = arithmetic(cs, j, inv, cur[0], cur[1], MOD[field])
        h = cs.add(h, cs.pow(d, (1 << 33) + 5))
        if chain:
            h = cs.add(h, cs.pow_chain(e, tmp_chain(3)))
        return [h, cur[0]]
    return WalkBody(2, 2, b)


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_a_the_round_kernels_equal_the_host_evaluator(ctx, field):
    m, rng = MOD[field], np.random.default_rng(11 + field)
    tape = record_round_body(round_body(field), field)
    assert sorted({op for op, *_ in tape.op_list()}) == list(range(9)) and tape.c.n_inv == 2
    nv, stride = tape.c.n_vars, N + 2
    inv, adv = elements(rng, 2 * LANES, m), elements(rng, 2 * ((LANES - 1) * stride + N + 1), m)
    d_adv = dev(adv)
    got = dev(guard(N * nv + 1))
    ctx.round_tape_run(field, tape, N, inv[:2], d_adv, got)
    got_l = dev(guard(LANES * N * nv + 1))
    ctx.round_tape_run_lanes(field, tape, N, LANES, inv, d_adv, stride, got_l)
    ctx.sync()
    want, want_l = guard(N * nv + 1), guard(LANES * N * nv + 1)
    want[:N * nv] = round_tape_eval(field, tape, N, inv[:2], adv)
    want_l[:LANES * N * nv] = round_tape_eval_lanes(field, tape, N, LANES, inv, adv, stride)
    assert host(got).tobytes() == want.tobytes()
    assert host(got_l).tobytes() == want_l.tobytes()
    assert want_l[:N * nv].tobytes() == want[:N * nv].tobytes() and want_l[N * nv:2 * N * nv].tobytes() != want[:N * nv].tobytes()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_a_the_descending_walks_equal_the_host_evaluator(ctx, field):
    import torch
    m, rng = MOD[field], np.random.default_rng(12 + field)
    tape = record_walk_body(walk_body(field), field)
    assert sorted({op for op, *_ in tape.op_list()}) == list(range(9)) and tape.c.n_inv == 2
    group, n_groups = 5, N // 5
    lay = dict(walk_stride=ROUNDS, top=ROUNDS, group=group, group_stride=group * ROUNDS + 2, j_group_step=1000, heads=True)
    n_trace = 2 * (n_groups * lay["group_stride"] + 1)
    inv, start = elements(rng, 2 * LANES, m), elements(rng, 2 * N, m)
    for lanes in (1, LANES):
        jb = [77, 2**64 - 1, 5 << 40][:lanes]
        def run(walk, entries, trace, expect, ok):
            if lanes == 1:
                walk(field, tape, inv[:2], entries, N, ROUNDS, trace, j_base=jb[0], expect=expect, ok=ok, **lay)
            else:
                walk(field, tape, lanes, inv, entries, N, ROUNDS, trace, j_base=jb, expect=expect, ok=ok, **lay)
        host_walk = walk_tape_eval if lanes == 1 else walk_tape_eval_lanes
        landing, want_tr = start.copy(), guard(n_trace)
        run(host_walk, landing, want_tr, None, None)
        expect = landing.copy()
        expect[2 * 64] ^= np.uint64(1)                           # the one walk of the second workgroup misses its checkpoint
        want_e, want_ok = start.copy(), np.full(N, -1, dtype="<i4")
        run(host_walk, want_e, want_tr, expect, want_ok)
        assert want_ok.tolist() == [1] * 64 + [0] and want_e.tobytes() == landing.tobytes()
        d_e, d_tr, d_ok = dev(start), dev(guard(n_trace)), torch.full((N,), -1, dtype=torch.int32, device="cuda")
        run(ctx.round_tape_walk if lanes == 1 else ctx.round_tape_walk_lanes, d_e, d_tr, dev(expect), d_ok)
        ctx.sync()
        assert host(d_e).tobytes() == want_e.tobytes()
        assert host(d_tr).tobytes() == want_tr.tobytes()
        assert d_ok.cpu().tolist() == want_ok.tolist()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("chain", [False, True])
def test_a_the_forward_walks_equal_the_host_evaluator(ctx, chain, field):
    m, rng = MOD[field], np.random.default_rng(13 + field)
    tape = record_forward_body(forward_body(field, chain), field)
    assert sorted({op for op, *_ in tape.op_list()}) == list(range(10 + chain)) and tape.c.n_inv == 2
    lay = dict(every=2, cp_stride=4, walk_stride=7, base=1, j_base=2**64 - 3, j_walk_step=1000)      # entries 2 .. 4, checkpoints 1 and 2
    inv, start = elements(rng, 2, m), elements(rng, 2 * N, m)
    want_e, want_cp, want_tr = start.copy(), guard(2 * (N * 4 + 1)), guard(2 * (N * 7 + 1))
    forward_tape_eval(field, tape, inv, want_e, N, ROUNDS, checkpoints=want_cp, trace=want_tr, **lay)
    d_e, d_cp, d_tr = dev(start), dev(guard(2 * (N * 4 + 1))), dev(guard(2 * (N * 7 + 1)))
    ctx.set_kernel_timing(True)
    ctx.kernel_events()
    ctx.round_tape_forward_walk(field, tape, inv, d_e, N, ROUNDS, checkpoints=d_cp, trace=d_tr, **lay)
    ctx.sync()
    names = [e[0] for e in ctx.kernel_events()]
    ctx.set_kernel_timing(False)
    assert names == ["k_tape_forward_walk_chain"[:23] if chain else "k_tape_forward_walk"]      # (an event's name holds 23 characters)
    assert host(d_e).tobytes() == want_e.tobytes()
    assert host(d_cp).tobytes() == want_cp.tobytes()
    assert host(d_tr).tobytes() == want_tr.tobytes()
    assert int((want_cp.reshape(-1, 8)[:, 0] != np.uint64(SENTINEL)).sum()) == 2 * N


def test_b_the_launchers_refuse_every_broken_rule_before_a_launch(ctx):
    field, m = FIELD_FQ, MOD[FIELD_FQ]
    inv = mont_rows([3], m)
    d_adv, d_out = dev(mont_rows([5, 6, 8, 9], m)), dev(guard(N_ADV))
    d_entries, d_trace, d_cp = dev(mont_rows([5, 6], m)), dev(guard(2 * N_ADV)), dev(guard(2 * N_ADV))
    before = [host(x).copy() for x in (d_out, d_entries, d_trace, d_cp)]

    def launch(mode, tape):
        if mode == ROUND:
            ctx.round_tape_run(field, tape, 1, inv, d_adv, d_out)
        elif mode == WALK:
            ctx.round_tape_walk(field, tape, inv, d_entries, 1, 1, d_trace, top=1, j_base=7, heads=True)
        else:
            ctx.round_tape_forward_walk(field, tape, inv, d_entries, 1, 1, d_cp, 1, 2, d_trace, 2, 0, j_base=7)
    ctx.set_kernel_timing(True)
    ctx.kernel_events()
    for name, modes, mutate, _names in cases():
        for mode in modes:
            tape = base_tape(mode, field)
            mutate(tape)
            with pytest.raises(VdfError) as e:
                launch(mode, tape)
            assert e.value.code == VDF_ERR_BAD_ARG, (name, mode, str(e.value))
    ctx.sync()
    assert ctx.kernel_events() == []
    assert [host(x).tobytes() for x in (d_out, d_entries, d_trace, d_cp)] == [b.tobytes() for b in before]
    # the valid tape of each mode launches, and lands where the host evaluator lands
    launch(ROUND, base_tape(ROUND, field))
    launch(FORWARD, base_tape(FORWARD, field))
    ctx.sync()
    assert sorted(e[0] for e in ctx.kernel_events()) == ["k_round_tape", "k_tape_forward_walk_chain"[:23]]
    ctx.set_kernel_timing(False)
    want_e, want_cp, want_tr = before[1].copy(), before[3].copy(), before[2].copy()
    forward_tape_eval(field, base_tape(FORWARD, field), inv, want_e, 1, 1, want_cp, 1, 2, want_tr, 2, 0, j_base=7)
    assert host(d_out).tobytes() == round_tape_eval(field, base_tape(ROUND, field), 1, inv, mont_rows([5, 6, 8, 9], m)).tobytes()
    assert (host(d_entries).tobytes(), host(d_cp).tobytes(), host(d_trace).tobytes()) == (want_e.tobytes(), want_cp.tobytes(), want_tr.tobytes())
