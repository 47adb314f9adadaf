"""CPU: VDF_TAPE_TAB and vdf_cs_tab on the host (include/vdf_hip.h, include/vdf_nova.h; tests/tab_spec.py states them as integers).

a. the rules (vdf_amd/csrc/tape_rules.h): every refusal of a TAB and of a table, in every mode, names the op or the table, and
   nothing is written; opcode 11 in a tape without a table stays a malformed op; the valid tape of each mode runs;
b. the recorder: vdf_cs_tab on a live vdf_cs and a second table set the failure flag, in all three kinds of body;
c. the five host evaluators against the spec for bodies that use every op together with TAB, tab_rows in {1, 3, 64, 65}, tab_cols
   in {1, 8}, entries 0 and m - 1 in the table, both fields, a counter that crosses 2^64 inside a walk in either direction;
d. a round body with a table has the shape and the digest of the plain loop with vdf_cs_const;
e. the chain constructors refuse a table whose rows do not divide t, or a j_base."""
import ctypes as C
import re

import numpy as np
import pytest

import tab_spec as ts
from oracle import pasta as o
from rounds_spec import MOD, mont_rows
from tape_rules_spec import FORWARD, MODES, N_ADV, ROUND, WALK, base_tape
from test_tape_rules_host import host_run
from util import ints
from vdf_amd._lib import VDF_ERR_BAD_ARG, VDF_OK
from vdf_amd.hip import TAPE_MAX_TAB_COLS, TAPE_MAX_TAB_ROWS, TAPE_TAB, VdfError
from vdf_amd.nova import (CustomChain, RoundBody, StepCircuit, WalkBody, forward_tape_eval, record_forward_body, record_round_body,
                          record_walk_body, round_tape_eval, round_tape_eval_lanes, shape_digest_custom, walk_tape_eval, walk_tape_eval_lanes,
                          FIELD_FP, FIELD_FQ)

FIELDS = [FIELD_FQ, FIELD_FP]
ROWS, COLS = [1, 3, 64, 65], [1, 8]
TAB_AT = 5            # op 5 of tape_rules_spec.base_ops is (CONST, 3, 0, 0): a TAB takes its place, same slot


def from_mont(arr, m):
    return [o.from_mont(v, m) for v in ints(arr)]


def table(rows, cols, field):
    m = MOD[field]
    vals = ts.table_ints(rows, cols, m)
    assert m - 1 in vals and (0 in vals or len(vals) == 1)         # (a table of one element holds m - 1)
    return vals, ts.table_array(vals, rows, cols, m)


# ---- a. the rules --------------------------------------------------------------------------------------------------------------
def tabbed_tape(mode, field=FIELD_FQ, rows=3, cols=2, col=1):
    tape = base_tape(mode, field)
    tape.set_table(table(rows, cols, field)[1])
    tape.ops[TAB_AT].op, tape.ops[TAB_AT].a, tape.ops[TAB_AT].b = TAPE_TAB, col, 0
    return tape


def _dims(rows, cols):
    def mutate(t):
        t.c.tab_rows, t.c.tab_cols = rows, cols
    return mutate


def _null(t):
    t.c.table = None


def _op(**f):
    def mutate(t):
        for k, v in f.items():
            setattr(t.ops[TAB_AT], k, v)
    return mutate


REFUSALS = [("a TAB in a tape without a table", _dims(0, 0), r"tape op %d\b.*malformed" % TAB_AT),
            ("a TAB of a column one past tab_cols", _op(a=2), r"tape op %d\b.*TAB" % TAB_AT),
            ("a TAB with b != 0", _op(b=1), r"tape op %d\b.*TAB" % TAB_AT),
            ("tab_rows = 0 beside tab_cols > 0", _dims(0, 2), "table"),
            ("tab_cols = 0 beside tab_rows > 0", _dims(3, 0), "table"),
            ("tab_rows one past its cap", _dims(TAPE_MAX_TAB_ROWS + 1, 2), "table.*cap"),
            ("tab_cols one past its cap", _dims(3, TAPE_MAX_TAB_COLS + 1), "table.*cap"),
            ("a null table with tab_rows > 0", _null, "null table")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,mutate,names", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_in_every_mode_names_the_op_or_the_table_and_nothing_is_written(name, mutate, names, mode):
    tape = tabbed_tape(mode)
    mutate(tape)
    rc, msg, before, after = host_run(mode, FIELD_FQ, tape)
    assert rc == VDF_ERR_BAD_ARG, (rc, msg)
    assert re.search(names, msg), msg
    assert all(np.array_equal(b, a) for b, a in zip(before, after))


@pytest.mark.parametrize("mode", MODES)
def test_opcode_11_in_a_tape_without_a_table_is_still_a_malformed_op(mode):
    """every tape that existed before the op has tab_rows = 0: for it opcode 11 is what it always was"""
    tape = base_tape(mode, FIELD_FQ)
    assert tape.c.tab_rows == 0 and tape.c.tab_cols == 0 and not tape.c.table
    tape.ops[TAB_AT].op = TAPE_TAB
    rc, msg, before, after = host_run(mode, FIELD_FQ, tape)
    assert rc == VDF_ERR_BAD_ARG and "malformed" in msg and re.search(r"tape op %d\b" % TAB_AT, msg), msg
    assert all(np.array_equal(b, a) for b, a in zip(before, after))


def test_the_table_rules_hold_in_the_lanes_evaluators_too():
    m = MOD[FIELD_FQ]
    inv = mont_rows([3, 4], m)
    tape = tabbed_tape(ROUND)
    tape.ops[TAB_AT].a = 2
    with pytest.raises(VdfError) as e:
        round_tape_eval_lanes(FIELD_FQ, tape, 1, 2, inv, mont_rows(list(range(8)), m), 2)
    assert e.value.code == VDF_ERR_BAD_ARG and "TAB" in str(e.value)
    tape = tabbed_tape(WALK)
    tape.c.table = None
    with pytest.raises(VdfError) as e:
        walk_tape_eval_lanes(FIELD_FQ, tape, 2, inv, mont_rows([5, 6, 7, 8], m), 2, 1, j_base=[0, 1])
    assert e.value.code == VDF_ERR_BAD_ARG and "null table" in str(e.value)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("mode", MODES)
def test_the_valid_tabbed_tape_of_each_mode_runs_and_reads_its_row(mode, field):
    """the hand-made tape with every op, its CONST replaced by a TAB: the run differs from the base tape's by exactly the change
    of that one value, checked through a second table whose row holds the constant itself"""
    m = MOD[field]
    want = host_run(mode, field, base_tape(mode, field))
    assert want[0] == VDF_OK
    # J = 0 in the round evaluator, 7 in both walks (host_run): with 3 rows, row 0 and row 1; put the constant 7 in both
    tape = tabbed_tape(mode, field)
    vals = [11, 7, 13, 7, 17, 19]
    tape.set_table(ts.table_array(vals, 3, 2, m))
    got = host_run(mode, field, tape)
    assert got[0] == VDF_OK, got[1]
    assert all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))
    # and the row of another J gives another result
    vals[1 if mode == ROUND else 3] = 8
    tape.set_table(ts.table_array(vals, 3, 2, m))
    other = host_run(mode, field, tape)
    assert other[0] == VDF_OK and not all(np.array_equal(a, b) for a, b in zip(other[3], want[3]))


# ---- b. the recorder -----------------------------------------------------------------------------------------------------------
def refused(f):
    with pytest.raises(VdfError) as e:
        f()
    assert e.value.code == VDF_ERR_BAD_ARG
    return str(e.value)


def test_a_table_is_legal_in_bodies_only_and_there_is_one_per_body():
    _, T = table(3, 2, FIELD_FQ)
    _, U = table(3, 2, FIELD_FQ)                                   # the same elements at another address
    assert T.tobytes() == U.tobytes() and T.ctypes.data != U.ctypes.data

    class Live(StepCircuit):                                       # a live vdf_cs: the failure flag, as vdf_cs_pow
        arity = 1

        def synthesize(self, cs, z):
            self.handle = cs.tab(T, 0)
            return [cs.mul(z[0], z[0])]
    live = Live()
    refused(lambda: shape_digest_custom(live))
    assert live.handle == 0
    # all three kinds of body take one, and name it in their tape; the same table twice is one table
    rb = RoundBody(0, 1, 1, lambda cs, j, inv, carry, cur, nx: [cs.mul(cs.add(carry[0], cs.tab(T, 0)), cs.tab(T, 1))])
    wb = WalkBody(0, 1, lambda cs, j, inv, e: [cs.add(cs.add(e[0], cs.tab(T, 0)), cs.tab(T, 1))])
    for tape in (record_round_body(rb), record_walk_body(wb), record_forward_body(wb)):
        assert tape.table is T and (tape.c.table, tape.c.tab_rows, tape.c.tab_cols) == (T.ctypes.data, 3, 2)
        assert [x[2] for x in tape.op_list() if x[0] == TAPE_TAB] == [0, 1] and tape.c.n_consts == 0
    # a second table -- another pointer, other rows, other cols -- a column past the table, dimensions past the caps
    two = lambda cs, a: cs.add(cs.add(a, cs.tab(T, 0)), cs.tab(U, 0))
    assert "table" in refused(lambda: record_round_body(RoundBody(0, 1, 1, lambda cs, j, inv, carry, cur, nx: [cs.mul(two(cs, carry[0]), carry[0])])))
    assert "table" in refused(lambda: record_walk_body(WalkBody(0, 1, lambda cs, j, inv, e: [two(cs, e[0])])))
    assert "table" in refused(lambda: record_forward_body(WalkBody(0, 1, lambda cs, j, inv, e: [two(cs, e[0])])))
    view = T[:2]                                                   # the same address with other rows
    refused(lambda: record_walk_body(WalkBody(0, 1, lambda cs, j, inv, e: [cs.add(cs.tab(T, 0), cs.tab(view, 0))])))
    refused(lambda: record_walk_body(WalkBody(0, 1, lambda cs, j, inv, e: [cs.add(e[0], cs.tab(T, 2))])))
    big = np.zeros((TAPE_MAX_TAB_ROWS + 1, 1, 4), dtype="<u8")
    refused(lambda: record_walk_body(WalkBody(0, 1, lambda cs, j, inv, e: [cs.add(e[0], cs.tab(big, 0))])))
    wide = np.zeros((1, TAPE_MAX_TAB_COLS + 1, 4), dtype="<u8")
    refused(lambda: record_walk_body(WalkBody(0, 1, lambda cs, j, inv, e: [cs.add(e[0], cs.tab(wide, 0))])))
    # at the caps it records
    full = np.zeros((TAPE_MAX_TAB_ROWS, TAPE_MAX_TAB_COLS, 4), dtype="<u8")
    t = record_walk_body(WalkBody(0, 1, lambda cs, j, inv, e: [cs.add(e[0], cs.tab(full, TAPE_MAX_TAB_COLS - 1))]))
    assert (t.c.tab_rows, t.c.tab_cols) == (TAPE_MAX_TAB_ROWS, TAPE_MAX_TAB_COLS)


def test_python_keeps_a_bodys_table_for_one_recording_only():
    """the tape keeps its array alive; the module keeps nothing, whether a recording returns, raises or never was one"""
    import gc
    import weakref
    from vdf_amd import nova
    _, T = table(3, 2, FIELD_FQ)
    tape = record_walk_body(WalkBody(0, 1, lambda cs, j, inv, e: [cs.add(e[0], cs.tab(T, 0))]))
    assert tape.table is T and nova._RECORDINGS == []

    def raising(cs, j, inv, e):
        cs.tab(T, 0)
        raise KeyError("the body's own")
    with pytest.raises(KeyError):
        record_walk_body(WalkBody(0, 1, raising))
    assert nova._RECORDINGS == []

    class Circuit(StepCircuit):                                    # cs.tab inside a live synthesize's repeat: no recording of Python's
        arity = 1

        def synthesize(self, cs, z):
            return cs.repeat(RoundBody(0, 1, 1, lambda c, j, inv, carry, cur, nx: [c.mul(carry[0], c.tab(T, 1))]), 3, [], z, None)
    shape_digest_custom(Circuit())
    assert nova._RECORDINGS == []
    ref = weakref.ref(T)
    del T, tape
    gc.collect()
    assert ref() is None


# ---- c. the five evaluators against the spec -----------------------------------------------------------------------------------
def _cols(cols):
    return (0, cols - 1)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_the_round_evaluators_against_the_spec(rows, cols, field):
    m = MOD[field]
    vals, T = table(rows, cols, field)
    c0, c1 = _cols(cols)
    tape = record_round_body(ts.round_body(field, T, c0, c1), field)
    ops = {x[0] for x in tape.op_list()}
    assert ops == {0, 1, 2, 3, 4, 5, 6, 7, 8, TAPE_TAB}            # every op of a round tape, and TAB
    t, lanes = 130, 3
    rng = np.random.default_rng(rows + cols)
    ks = [9, 0, m - 1]
    advs = [ts.round_advice(5 + l, ks[l], t, m, rng, vals, rows, cols, c0, c1) for l in range(lanes)]
    want = [ts.round_vars(advs[l], t, [ks[l]], m, vals, rows, cols, c0, c1) for l in range(lanes)]
    got = round_tape_eval(field, tape, t, mont_rows(ks[:1], m), mont_rows(advs[0], m))
    assert from_mont(got, m) == want[0]
    stride = t + 2
    flat = []
    for a in advs:
        flat += a + [0] * 3
    got = round_tape_eval_lanes(field, tape, t, lanes, mont_rows(ks, m), mont_rows(flat, m), stride)
    assert from_mont(got, m) == want[0] + want[1] + want[2]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_the_walk_evaluators_against_the_spec_also_across_the_wrap(rows, cols, field):
    m = MOD[field]
    vals, T = table(rows, cols, field)
    c0, c1 = _cols(cols)
    tape = record_walk_body(ts.walk_body(field, T, c0, c1), field)
    assert {x[0] for x in tape.op_list()} == {0, 1, 2, 3, 4, 5, 6, 7, 8, TAPE_TAB}
    fn = lambda cur, J, inv, mm: ts.walk_ints(cur, J, inv, mm, vals, rows, cols, c0, c1)
    n, rounds, lay = 4, 7, dict(walk_stride=7, top=7, group=2, group_stride=16, j_group_step=1000)
    start = [int(v) for v in np.random.default_rng(rows).integers(1, 2**62, size=n * 3)]
    start[1], start[5] = 0, m - 1
    for j_base in (0, 2**64 - 5, 2**64 - 1003):                   # the second and the third cross 2^64 inside a walk
        land, trace = list(start), [0] * (3 * 32)
        ts.model_walk(fn, m, 3, [99], land, n, rounds, trace=trace, j_base=j_base, heads=True, **lay)
        e, tr = mont_rows(start, m), mont_rows([0] * (3 * 32), m)
        walk_tape_eval(field, tape, mont_rows([99], m), e, n, rounds, trace=tr, j_base=j_base, heads=True, **lay)
        assert from_mont(e, m) == land and from_mont(tr, m) == trace, j_base
    # in lanes: two lanes whose j_base differ modulo rows (when there is more than one row), one of them across the wrap
    jb, inv = [2**64 - 3, 5], [99, 98]
    land, trace = list(start), [0] * (3 * 32)
    ts.model_walk(fn, m, 3, inv, land, n, rounds, trace=trace, walk_stride=7, top=7, group=1, group_stride=8, j_base=jb, j_group_step=1000,
                  heads=True, lanes=2)
    e, tr = mont_rows(start, m), mont_rows([0] * (3 * 32), m)
    walk_tape_eval_lanes(field, tape, 2, mont_rows(inv, m), e, n, rounds, trace=tr, walk_stride=7, top=7, group=1, group_stride=8, j_base=jb,
                         j_group_step=1000, heads=True)
    assert from_mont(e, m) == land and from_mont(tr, m) == trace


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_the_forward_evaluator_against_the_spec_also_across_the_wrap(rows, cols, field):
    m = MOD[field]
    vals, T = table(rows, cols, field)
    c0, c1 = _cols(cols)
    tape = record_forward_body(ts.forward_body(field, T, c0, c1, chain=True), field)
    assert {x[0] for x in tape.op_list()} == set(range(12))         # every op there is
    fn = lambda cur, J, inv, mm: ts.forward_ints(cur, J, inv, mm, vals, rows, cols, c0, c1, True)
    n, rounds = 3, 7
    start = [int(v) for v in np.random.default_rng(rows).integers(1, 2**62, size=n * 3)]
    start[1], start[5] = 0, m - 1
    for j_base in (0, 2**64 - 5):
        land, trace, cps = list(start), [0] * (3 * 3 * 11), [0] * (3 * 3 * 4)
        ts.model_forward(fn, m, 3, [99], land, n, rounds, checkpoints=cps, every=3, cp_stride=4, trace=trace, walk_stride=11, base=2,
                         j_base=j_base, j_walk_step=1000)
        e, tr, cp = mont_rows(start, m), mont_rows([0] * len(trace), m), mont_rows([0] * len(cps), m)
        forward_tape_eval(field, tape, mont_rows([99], m), e, n, rounds, checkpoints=cp, every=3, cp_stride=4, trace=tr, walk_stride=11,
                          base=2, j_base=j_base, j_walk_step=1000)
        assert from_mont(e, m) == land and from_mont(tr, m) == trace and from_mont(cp, m) == cps, j_base


def test_the_evaluators_with_a_table_at_the_caps():
    field, m = FIELD_FQ, MOD[FIELD_FQ]
    rows, cols = TAPE_MAX_TAB_ROWS, TAPE_MAX_TAB_COLS
    vals, T = table(rows, cols, field)
    tape = record_forward_body(ts.forward_body(field, T, 0, cols - 1), field)
    fn = lambda cur, J, inv, mm: ts.forward_ints(cur, J, inv, mm, vals, rows, cols, 0, cols - 1)
    land = [1, 2, 3]
    ts.model_forward(fn, m, 3, [99], land, 1, 4, j_base=rows - 2)     # rows - 2, rows - 1, 0, 1
    e = mont_rows([1, 2, 3], m)
    forward_tape_eval(field, tape, mont_rows([99], m), e, 1, 4, j_base=rows - 2)
    assert from_mont(e, m) == land


# ---- d. shape and digest -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("rows", [1, 3, 4])
def test_a_tabbed_round_has_the_shape_and_the_digest_of_the_plain_loop(rows, field):
    vals, T = table(rows, 2, field)
    rep = shape_digest_custom(ts.TM(8, T, vals, "repeat", field))
    loop = shape_digest_custom(ts.TM(8, T, vals, "loop", field))
    assert rep[0] == loop[0] and np.array_equal(rep[1], loop[1])
    other = list(vals)
    other[-1] = (other[-1] + 1) % MOD[field]                       # one element of the table: another circuit
    assert shape_digest_custom(ts.TM(8, ts.table_array(other, rows, 2, MOD[field]), other, "repeat", field))[0] != rep[0]


# ---- e. chains -----------------------------------------------------------------------------------------------------------------
def test_the_chain_constructors_refuse_rows_that_do_not_divide_t_or_a_j_base():
    field, m = FIELD_FQ, MOD[FIELD_FQ]
    vals, T = table(4, 2, field)
    tape = record_walk_body(ts.minroot_walk_body(field, T, 0, 1), field)
    cps = mont_rows(list(range(2 * 7)), m)                          # 3 steps x 2 intervals + 1 entries of (x, y)
    good = CustomChain.from_checkpoints(field, tape, None, 8, 4, 3, cps)
    assert good.host_bytes() >= 4 * 2 * 32 + cps.nbytes             # the table's copy is counted
    good.free()
    CustomChain.from_checkpoints(field, tape, None, 8, 4, 3, cps, j_base=2**64 - 4).free()
    msg = refused(lambda: CustomChain.from_checkpoints(field, tape, None, 6, 3, 3, mont_rows(list(range(14)), m)))
    assert "tab_rows must divide t" in msg
    msg = refused(lambda: CustomChain.from_checkpoints(field, tape, None, 8, 4, 3, cps, j_base=6))
    assert "tab_rows must divide every j_base" in msg
    lanes_cps = mont_rows(list(range(2 * 7 * 2)), m)
    msg = refused(lambda: CustomChain.lanes_from_checkpoints(field, tape, None, 8, 4, 3, 2, lanes_cps, 7, j_base=[8, 9]))
    assert "tab_rows must divide every j_base" in msg
    CustomChain.lanes_from_checkpoints(field, tape, None, 8, 4, 3, 2, lanes_cps, 7, j_base=[8, 12]).free()
