"""CPU tests of traces rebuilt by forward tapes: the host restatement vdf_nova_forward_tape_rebuild_eval_lanes against whole chains
walked from entry 0 (forward_rebuild_spec: independent of the new index rule), every refusal by its message, and what the ascending
chain object says on the host -- its constructors' refusals, its direction and the clamp of launch_rounds."""
import numpy as np
import pytest

import forward_rebuild_spec as fs
from forward_rebuild_spec import EVERY, IDS, MATRIX, ROWS, STEPS, case, run_window
import walks_spec
from pow_chain_spec import tmp_chain
from rounds_spec import MOD, fe, mont_rows
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.minroot import pow_chain as minroot_pow_chain
from vdf_amd.nova import (CHAIN_ASCENDING, CHAIN_DESCENDING, CustomChain, WalkBody, forward_tape_rebuild_eval_lanes, record_forward_body,
                          record_walk_body, FIELD_FP, FIELD_FQ)

@pytest.mark.parametrize("field,na,lanes,group,heads,tab", MATRIX, ids=IDS)
def test_the_restatement_rebuilds_the_windows_of_whole_chains(field, na, lanes, group, heads, tab):
    tape, inv, jb, chains, t = case(field, na, lanes, group, tab)
    lo, hi = fs.window(chains, na, t, EVERY, 0, STEPS)
    n, stride = STEPS * lanes * group, t + 2
    trace = np.full((n // group * stride * na, 4), fs.FILL, dtype="<u8")
    ok = np.full(n, -7, dtype="<i4")
    entries = run_window(forward_tape_rebuild_eval_lanes, field, tape, lanes, inv, jb, lo, hi, trace, ok, t, group, heads, stride)
    assert entries.tobytes() == hi.tobytes()
    assert ok.tolist() == [1] * n
    assert trace.tobytes() == fs.window_traces(chains, na, t, 0, STEPS, stride, bool(heads)).tobytes()


def test_the_bodies_are_their_big_integer_statements():
    for field in (FIELD_FQ, FIELD_FP):
        m = MOD[field]
        vals, T = fs.rescue_table(field, 4)
        tape = record_forward_body(fs.rescue_forward_body(field, T), field)
        got = fs.tape_ints(fs.chain_trace(field, tape, None, mont_rows([5, m - 1, 0, 0], m), 9, j_base=2**64 - 3), m)
        cur = [5, m - 1, 0, 0]
        for k in range(9):
            cur = fs.rescue_forward_ints(cur, 2**64 - 3 + k, m, vals, 4)
            assert got[4 * (k + 1):4 * (k + 2)] == cur
        xt = [11 + 5 * r + c for r in range(ROWS) for c in range(2)]
        X = record_forward_body(fs.every_op_body(field, 4, np.ascontiguousarray(mont_rows(xt, m).reshape(ROWS, 2, 4))), field)
        got = fs.tape_ints(fs.chain_trace(field, X, mont_rows([9], m), mont_rows([1, 2, 3, m - 1], m), 7, j_base=2**64 - 3), m)
        cur = [1, 2, 3, m - 1]
        for k in range(7):
            cur = fs.every_op_ints(cur, (2**64 - 3 + k) % 2**64, [9], m, 4, xt, ROWS, 2)
            assert got[4 * (k + 1):4 * (k + 2)] == cur


def test_a_planted_wrong_expect_is_a_result_and_group_zero_is_one_group():
    field, na = FIELD_FQ, 2
    tape, inv, jb, chains, t = case(field, na, 1, 2, False)
    lo, hi = fs.window(chains, na, t, EVERY, 0, STEPS)
    bad = hi.copy()
    bad[2 * na + 1, 3] ^= np.uint64(1 << 40)
    ok = np.full(4, -7, dtype="<i4")
    entries = lo.copy()
    forward_tape_rebuild_eval_lanes(field, tape, 1, inv, entries, 4, EVERY, walk_stride=EVERY, group=2, group_stride=t + 1, j_base=jb, j_group_step=t,
                                    expect=bad, ok=ok)
    assert ok.tolist() == [1, 1, 0, 1] and entries.tobytes() == hi.tobytes()
    # group = 0: every walk is group 0 of step 0 -- the first step's two walks alone, group_stride ignored
    trace = np.full(((t + 1) * na, 4), fs.FILL, dtype="<u8")
    entries = lo[:2 * na].copy()
    forward_tape_rebuild_eval_lanes(field, tape, 1, inv, entries, 2, EVERY, trace=trace, walk_stride=EVERY, group=0, group_stride=12345, j_base=jb,
                                    j_group_step=777, heads=True)
    assert trace.tobytes() == chains[0][:(t + 1) * na].tobytes()
    # n = 0 and rounds = 0 do nothing
    forward_tape_rebuild_eval_lanes(field, tape, 1, inv, None, 0, 5, j_base=jb)
    before = entries.copy()
    forward_tape_rebuild_eval_lanes(field, tape, 1, inv, entries, 2, 0, j_base=jb)
    assert entries.tobytes() == before.tobytes()


def refused(text, *args, **kw):
    with pytest.raises(VdfError) as e:
        forward_tape_rebuild_eval_lanes(*args, **kw)
    assert e.value.code == VDF_ERR_BAD_ARG and text in str(e.value), str(e.value)


def test_every_refusal_by_its_message():
    field, m = FIELD_FQ, MOD[FIELD_FQ]
    X = record_forward_body(fs.every_op_body(field, 2), field)
    inv, e = mont_rows([9] * 16, m), np.zeros((8 * 2, 4), dtype="<u8")
    tr, ok = np.zeros((64, 4), dtype="<u8"), np.zeros(8, dtype="<i4")
    # the rules of a forward walk tape, through the one statement of them
    refused("a forward walk tape loads advice with b = 0 only", field, record_walk_body(walks_spec.minroot_body(field), field), 1, inv, e, 1, 1)
    refused("unknown field", 7, X, 1, inv, e, 1, 1)
    # the lanes
    refused("lanes must be 1 .. VDF_TAPE_MAX_LANES", field, X, 0, inv, e, 1, 1)
    refused("lanes must be 1 .. VDF_TAPE_MAX_LANES", field, X, 17, inv, e, 1, 1)
    six = record_forward_body(WalkBody(6, 2, lambda cs, j, inv, cur: [cs.add(cur[0], inv[5]), cur[0]]), field)
    refused("lanes * n_inv > VDF_TAPE_MAX_INV", field, six, 3, np.zeros((18, 4), dtype="<u8"), e, 1, 1)
    refused("null j_base", field, X, 1, inv, e, 1, 1, j_base=False)
    refused("expect without ok", field, X, 1, inv, e, 1, 1, expect=e)
    # a walk that would write into the run of the walk above it: only with a trace and more than one walk per group
    refused("base + rounds > walk_stride", field, X, 1, inv, e, 4, 3, trace=tr, walk_stride=5, base=3, group=2, group_stride=11)
    forward_tape_rebuild_eval_lanes(field, X, 1, inv, e, 4, 3, walk_stride=5, base=3, group=2, group_stride=11)             # no trace
    forward_tape_rebuild_eval_lanes(field, X, 1, inv, e, 4, 3, trace=tr, walk_stride=5, base=3, group=1, group_stride=7)    # one walk per group
    # the slots: 8 columns twice, the live values, and a chain of as many temporaries as still fit -- then the 6 invariants do not
    def wide(n_tmp):
        def b(cs, j, inv, cur):
            s = cur[0]
            for k in range(6):
                s = cs.add(s, inv[k])
            return [cs.pow_chain(s, tmp_chain(n_tmp))] + [cur[i] for i in range(1, 8)]
        return record_forward_body(WalkBody(6, 8, b), field)
    room = fs.WALK_MAX_SLOTS - 16 - wide(2).c.n_slots
    assert 2 <= room <= 12
    big = wide(room)
    assert big.c.n_slots + 16 + room == fs.WALK_MAX_SLOTS
    refused("n_slots + 2 * n_adv + n_inv + the chains' n_tmp > VDF_WALK_MAX_SLOTS", field, big, 1, inv, np.zeros((8, 4), dtype="<u8"), 1, 1)
    # the work of one call: X spends 3 + 3 + 1 products per round
    most = fs.FORWARD_TAPE_MAX_WORK // 7
    refused("rounds x products per round > VDF_FORWARD_TAPE_MAX_WORK", field, X, 1, inv, None, 0, most + 1)
    forward_tape_rebuild_eval_lanes(field, X, 1, inv, None, 0, most)
    refused("null entries", field, X, 1, inv, None, 1, 1)


def pow_products(e):
    return e.bit_length() - 1 + bin(e).count("1") - 1


def test_the_constructors_the_direction_and_the_clamp_of_launch_rounds():
    field, m = FIELD_FQ, MOD[FIELD_FQ]
    vals, T = fs.rescue_table(field, 4)
    fwd = record_forward_body(fs.rescue_forward_body(field, T), field)
    cps = np.zeros(((3 * 2 + 1) * 4, 4), dtype="<u8")
    chain = CustomChain.from_checkpoints(field, fwd, None, 8, 4, 3, cps, forward=True)
    assert chain.direction == CHAIN_ASCENDING and len(chain) == 3 and chain.memory() == (0, 0)
    # two fifth roots by the library's chain and ten more products: the bound is 1,024, and nothing is refused above it
    assert chain.launch_rounds(0) == 1024 and chain.launch_rounds(5000) == 1024 and chain.launch_rounds(7) == 7
    chain.set_launch_rounds(3)
    assert chain.launch_rounds(0) == 3 and chain.launch_rounds(9) == 9
    chain.free()
    lanes = CustomChain.lanes_from_checkpoints(field, fwd, None, 8, 4, 3, 3, np.zeros((3 * 7 * 4, 4), dtype="<u8"), forward=True)
    assert lanes.direction == CHAIN_ASCENDING and lanes.lanes == 3
    lanes.free()
    # a tape of three square-and-multiply roots: VDF_FORWARD_TAPE_MAX_WORK / products is below 1,024
    e = pow(5, -1, m - 1)
    heavy = record_forward_body(WalkBody(0, 3, lambda cs, j, inv, cur: [cs.pow(c, e) for c in cur]), field)
    bound = fs.FORWARD_TAPE_MAX_WORK // (3 * pow_products(e))
    assert 0 < bound < 1024
    chain = CustomChain.from_checkpoints(field, heavy, None, 8, 4, 1, np.zeros((3 * 3, 4), dtype="<u8"), forward=True)
    assert chain.launch_rounds(0) == bound and chain.launch_rounds(1024) == bound and chain.launch_rounds(bound - 1) == bound - 1
    chain.free()
    # a descending chain keeps what it is asked for (0: the slicing rule's 1,024)
    walk = record_walk_body(walks_spec.minroot_body(field), field)
    chain = CustomChain.from_checkpoints(field, walk, mont_rows([0], m), 8, 4, 1, np.zeros((3 * 2, 4), dtype="<u8"))
    assert chain.direction == CHAIN_DESCENDING and chain.launch_rounds(0) == 0 and chain.launch_rounds(5000) == 5000
    chain.free()

    def no(text, tape, *args, **kw):
        with pytest.raises(VdfError) as err:
            CustomChain.from_checkpoints(field, tape, *args, forward=True, **kw).free()
        assert err.value.code == VDF_ERR_BAD_ARG and text in str(err.value), str(err.value)
    no("a forward walk tape loads advice with b = 0 only", walk, mont_rows([0], m), 8, 4, 1, np.zeros((3 * 2, 4), dtype="<u8"))
    no("`every` must be positive and divide t", fwd, None, 8, 3, 3, cps)
    no("t out of range", fwd, None, 0, 4, 3, cps)
    no("num_steps must be > 0", fwd, None, 8, 4, 0, cps)
    no("tab_rows must divide t", fwd, None, 6, 3, 3, np.zeros(((3 * 2 + 1) * 4, 4), dtype="<u8"))
    no("tab_rows must divide every j_base", fwd, None, 8, 4, 3, cps, j_base=6)
    with pytest.raises(VdfError) as err:
        CustomChain.lanes_from_checkpoints(field, fwd, None, 8, 4, 3, 17, cps, forward=True)
    assert "lanes must be 1 .. VDF_TAPE_MAX_LANES" in str(err.value)
    # and the descending constructor still refuses a tape that holds a power
    with pytest.raises(VdfError) as err:
        CustomChain.from_checkpoints(field, fwd, None, 8, 4, 3, cps)
    assert err.value.code == VDF_ERR_BAD_ARG
