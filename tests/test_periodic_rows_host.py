"""CPU: the periodic rows of a custom circuit's vdf_cs_repeat (include/vdf_hip.h vdf_periodic_rows, include/vdf_nova.h
vdf_nova_periodic_rows_detect / _eval / vdf_nova_shape_periodic_custom): the detection on the spec circuits and on hand-made
triples, the host evaluator against a big-integer sparse product over the exported triples, and its refusals.  Exact throughout."""
import numpy as np
import pytest

from oracle import pasta as o
from periodic_spec import GUARD, NUM_IO, described, guarded, operands, refusal_cases, sparse_reference
from rounds_spec import F, MOD, mont_rows
from util import ints
from vdf_amd.hip import (PERIODIC_MAX_CONSTS, PERIODIC_MAX_ROW_TERMS, PERIODIC_MAX_ROWS, PERIODIC_MAX_TERMS, TERM_ABS, TERM_NO_SLOPE,
                         TERM_SEG, VdfError)
from vdf_amd.nova import (FIELD_FP, FIELD_FQ, periodic_rows_detect, periodic_rows_eval, shape_digest_custom, shape_periodic_custom,
                          tuning_default)

FIELDS = [FIELD_FQ, FIELD_FP]


def const_ints(pr, field):
    return [o.from_mont(v, MOD[field]) for v in ints(pr.consts[:pr.c.n_consts])]


# ---- detection on the spec circuits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_the_forward_round_is_periodic_from_repetition_two(field):
    mats, pr, info = described("F", 5, field)
    assert pr is not None and pr.lead == 2 and (pr.c.n_cons, pr.c.n_vars, pr.c.n_terms, pr.c.j0) == (3, 3, 12, 2)
    assert pr.row_count == 3 * 3 and pr.row_begin + pr.row_count <= info["num_cons"]
    k = const_ints(pr, field)
    rows = pr.term_list()
    one_col, i_in = info["num_cols"] - 1 - NUM_IO, info["seg_begin"] - 1
    # x' x' = t1; t1 t1 = t2: copies of the repetition's own variables, coefficient 1
    assert [[[(kd, col, k[c0], c1) for kd, col, c0, c1 in mat] for mat in row] for row in rows[:2]] == [
        [[(TERM_SEG, 0, 1, TERM_NO_SLOPE)], [(TERM_SEG, 0, 1, TERM_NO_SLOPE)], [(TERM_SEG, 1, 1, TERM_NO_SLOPE)]],
        [[(TERM_SEG, 1, 1, TERM_NO_SLOPE)], [(TERM_SEG, 1, 1, TERM_NO_SLOPE)], [(TERM_SEG, 2, 1, TERM_NO_SLOPE)]]]
    # t2 x' = x_j + x_(j-1) + i_in + (j - 1) one: x' of repetitions j - 1 and j - 2, and the one affine term, slope 1
    a, b, c = rows[2]
    assert [(kd, col, k[c0]) for kd, col, c0, _ in a + b] == [(TERM_SEG, 2, 1), (TERM_SEG, 0, 1)]
    assert sorted((kd, col, k[c0], None if c1 == TERM_NO_SLOPE else k[c1]) for kd, col, c0, c1 in c) == sorted(
        [(TERM_SEG, -3, 1, None), (TERM_SEG, -6, 1, None), (TERM_ABS, i_in, 1, None), (TERM_ABS, one_col, 1, 1)])
    assert sum(c1 != TERM_NO_SLOPE for row in rows for mat in row for _, _, _, c1 in mat) == 1


@pytest.mark.parametrize("field", FIELDS)
def test_the_round_of_every_op_is_periodic_from_repetition_one(field):
    _, pr, _ = described("G", 5, field)
    assert pr is not None and pr.lead == 1 and (pr.c.n_cons, pr.c.n_vars) == (4, 5) and pr.row_count == 4 * 4


@pytest.mark.parametrize("field", FIELDS)
def test_fewer_than_two_periodic_repetitions_is_none(field):
    assert described("F", 3, field)[1] is None          # lead 2 leaves one repetition
    assert described("F", 4, field)[1] is not None


@pytest.mark.parametrize("field", FIELDS)
def test_a_carry_that_accumulates_is_not_periodic(field):
    assert described("Acc", 5, field)[1] is None and described("Acc", 12, field)[1] is None


def test_a_circuit_without_a_repeat_has_none():
    pr, info = shape_periodic_custom(F(5, "loop"))
    assert pr is None and info["seg_begin"] == 0 and info["num_cons"] == described("F", 5, FIELD_FQ)[2]["num_cons"]


# ---- hand-made triples ----------------------------------------------------------------------------------------------------------
SEG, NV, ROW0, T_BAND = 10, 2, 7, 6
ABS_COL, ONE_COL = 3, 40


def band(t=T_BAND, n_cons=2, extra=None):
    """rows of t repetitions, two variables each from column SEG: row 0  A = v0, B = v1, C = 5 v0(j) - v1(j - 1) + 2 x_3;
    row 1  A = v1, B = x_3, C = (3 + 2 j) one.  Repetition 0 has no look-back: lead 1.  -> {matrix: [(row, col, int)]}"""
    m = {0: [], 1: [], 2: []}
    for j in range(t):
        r, v = ROW0 + n_cons * j, SEG + NV * j
        m[0] += [(r, v, 1), (r + 1, v + 1, 1)]
        m[1] += [(r, v + 1, 1), (r + 1, ABS_COL, 1)]
        m[2] += [(r, v, 5), (r, ABS_COL, 2), (r + 1, ONE_COL, 3 + 2 * j)]
        if j:
            m[2].append((r, v - NV + 1, -1))
    if extra:
        extra(m)
    return m


def triples(m, field=FIELD_FQ):
    return [(np.array([e[0] for e in m[k]], dtype=np.uint32), np.array([e[1] for e in m[k]], dtype=np.uint32),
             mont_rows([e[2] for e in m[k]], MOD[field]).reshape(-1, 4)) for k in range(3)]


def detect(m, t=T_BAND, n_cons=2, n_vars=NV, field=FIELD_FQ):
    return periodic_rows_detect(field, triples(m, field), SEG, n_vars, ROW0, n_cons, t)


@pytest.mark.parametrize("field", FIELDS)
def test_a_periodic_band_is_accepted(field):
    pr = detect(band(), field=field)
    assert pr is not None and (pr.lead, pr.row_begin, pr.row_count) == (1, ROW0 + 2, 2 * (T_BAND - 1))
    k = const_ints(pr, field)
    m = MOD[field]
    c0 = sorted((kd, col, k[a], None if b == TERM_NO_SLOPE else k[b]) for kd, col, a, b in pr.term_list()[0][2])
    assert c0 == sorted([(TERM_SEG, 0, 5, None), (TERM_SEG, -1, m - 1, None), (TERM_ABS, ABS_COL, 2, None)])
    assert [(kd, col, k[a], k[b]) for kd, col, a, b in pr.term_list()[1][2]] == [(TERM_ABS, ONE_COL, 5, 2)]      # 3 + 2 j at j0 = 1


def change(matrix, index, **kw):
    def f(m):
        r, c, v = m[matrix][index]
        m[matrix][index] = (kw.get("row", r), kw.get("col", c), kw.get("val", v))
    return f


def test_one_coefficient_off_in_the_last_repetition_is_refused():
    last_c = len(band()[2]) - 4                            # 5 v0 of the last repetition
    assert band()[2][last_c] == (ROW0 + 2 * (T_BAND - 1), SEG + NV * (T_BAND - 1), 5)
    assert detect(band(extra=change(2, last_c, val=6))) is None
    assert detect(band(extra=change(0, len(band()[0]) - 1, val=2))) is None
    assert detect(band()) is not None


def test_a_column_moved_by_one_is_refused():
    # (in repetition 4 of 6: a lead of 4 would otherwise leave two repetitions that agree)
    mid = next(i for i, e in enumerate(band()[2]) if e[0] == ROW0 + 2 * 4 and e[2] == 5)
    assert detect(band(extra=change(2, mid, col=SEG + NV * 4 + 1))) is None               # the repetition's other variable
    idx = next(i for i, e in enumerate(band()[1]) if e[0] == ROW0 + 2 * 4 + 1)
    assert detect(band(extra=change(1, idx, col=ABS_COL + 1))) is None                     # a fixed column that moves


def test_a_slope_that_fits_two_repetitions_only_is_refused():
    def bend(m):
        for i, (r, c, v) in enumerate(m[2]):
            j = (r - ROW0) // 2
            if c == ONE_COL and j >= 3:
                m[2][i] = (r, c, v + (j - 2) ** 2)         # 3 + 2 j up to j = 2, then off every line: no lead in 0 .. 4 fits to the end
    assert detect(band(t=8, extra=bend), t=8) is None
    assert detect(band(t=8), t=8) is not None


def wide_row(n_terms):
    """one row per repetition whose C has n_terms terms: its own variable and n_terms - 1 fixed columns"""
    def f(t=4):
        m = {0: [], 1: [], 2: []}
        for j in range(t):
            m[0].append((ROW0 + j, SEG + j, 1))
            m[1].append((ROW0 + j, SEG + j, 1))
            m[2] += [(ROW0 + j, SEG + j, 1)] + [(ROW0 + j, 100 + q, 1) for q in range(n_terms - 1)]
        return m
    return f


def test_a_row_of_nine_terms_is_refused_and_eight_accepted():
    assert PERIODIC_MAX_ROW_TERMS == 8
    assert periodic_rows_detect(FIELD_FQ, triples(wide_row(8)()), SEG, 1, ROW0, 1, 4) is not None
    assert periodic_rows_detect(FIELD_FQ, triples(wide_row(9)()), SEG, 1, ROW0, 1, 4) is None


def many(n_cons, terms_in_c, n_consts=1, t=3):
    """n_cons rows per repetition, A = B = the repetition's variable; C of row c has terms_in_c[c] fixed columns whose coefficients
    run through n_consts distinct values (1 first)"""
    m = {0: [], 1: [], 2: []}
    for j in range(t):
        q = 0
        for c in range(n_cons):
            r = ROW0 + n_cons * j + c
            m[0].append((r, SEG + j, 1))
            m[1].append((r, SEG + j, 1))
            for e in range(terms_in_c[c]):
                m[2].append((r, 100 + e, 1 + q % n_consts))
                q += 1
    return m


def test_every_cap_is_accepted_at_the_cap_and_refused_one_beyond():
    det = lambda m, n_cons: periodic_rows_detect(FIELD_FQ, triples(m), SEG, 1, ROW0, n_cons, 3)
    # rows per repetition
    assert det(many(PERIODIC_MAX_ROWS, [1] * PERIODIC_MAX_ROWS), PERIODIC_MAX_ROWS) is not None
    assert det(many(PERIODIC_MAX_ROWS + 1, [1] * (PERIODIC_MAX_ROWS + 1)), PERIODIC_MAX_ROWS + 1) is None
    # terms per repetition: 2 per row in A and B, the rest in C
    n = 16
    at_cap = [4] * n                                       # 16 * (2 + 4) = 96 ... + 32 more
    for c in range(8):
        at_cap[c] = 8
    assert n * 2 + sum(at_cap) == PERIODIC_MAX_TERMS
    pr = det(many(n, at_cap), n)
    assert pr is not None and pr.c.n_terms == PERIODIC_MAX_TERMS
    beyond = list(at_cap)
    beyond[8] = 5
    assert det(many(n, beyond), n) is None
    # constants
    pr = det(many(4, [8] * 4, PERIODIC_MAX_CONSTS), 4)
    assert pr is not None and pr.c.n_consts == PERIODIC_MAX_CONSTS
    assert det(many(4, [8] * 4, PERIODIC_MAX_CONSTS + 1), 4) is None


# ---- the evaluator against a big-integer sparse product ---------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("t", [5, 65])
@pytest.mark.parametrize("name", ["F", "G"])
def test_the_evaluator_equals_the_sparse_product_over_the_exported_triples(name, t, field):
    mats, pr, info = described(name, t, field)
    z2, a1, b1, c1, u1 = operands(field, info, pr, seed=t + 7 * field)
    got = guarded(info["num_cons"])
    periodic_rows_eval(field, pr, pr.lead, t - pr.lead, info["seg_begin"], pr.row_begin, info["num_cols"], info["num_cons"], z2, a1, b1,
                       c1, u1, *got)
    want = sparse_reference(field, mats, pr.row_begin, pr.row_count, z2, a1, b1, c1, u1)
    lo, hi = pr.row_begin, pr.row_begin + pr.row_count
    for g, w in zip(got, want):
        assert g[lo:hi].tobytes() == w.tobytes()
        assert (g[:lo] == GUARD).all() and (g[hi:] == GUARD).all()
    # a part of the range: the repetitions from the third periodic one on
    if t - pr.lead > 3:
        part = guarded(info["num_cons"])
        skip = 2 * pr.c.n_cons
        periodic_rows_eval(field, pr, pr.lead + 2, t - pr.lead - 2, info["seg_begin"], pr.row_begin + skip, info["num_cols"],
                           info["num_cons"], z2, a1, b1, c1, u1, *part)
        for g, w in zip(part, want):
            assert g[lo + skip:hi].tobytes() == w[skip:].tobytes() and (g[:lo + skip] == GUARD).all() and (g[hi:] == GUARD).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_the_evaluator_refuses_a_malformed_description_and_then_runs_a_valid_one():
    t, field = 5, FIELD_FQ
    mats, pr, info = described("F", t, field)
    z2, a1, b1, c1, u1 = operands(field, info, pr, seed=1)
    want = guarded(info["num_cons"])
    call = dict(j_first=pr.lead, reps=t - pr.lead, seg_begin=info["seg_begin"], row_begin=pr.row_begin, num_cols=info["num_cols"],
                num_cons=info["num_cons"])
    periodic_rows_eval(field, pr, *call.values(), z2, a1, b1, c1, u1, *want)
    for name, mutate, over in refusal_cases(pr, info, t):
        undo = mutate()
        got = guarded(info["num_cons"])
        with pytest.raises(VdfError) as e:
            periodic_rows_eval(field, pr, *{**call, **over}.values(), z2, a1, b1, c1, u1, *got)
        assert e.value.code == 1, name                    # VDF_ERR_BAD_ARG
        assert all((g == GUARD).all() for g in got), name
        undo()
        periodic_rows_eval(field, pr, *call.values(), z2, a1, b1, c1, u1, *got)
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want], name
    none = guarded(info["num_cons"])
    periodic_rows_eval(field, pr, *{**call, "reps": 0}.values(), z2, a1, b1, c1, u1, *none)      # reps = 0 does nothing
    assert all((g == GUARD).all() for g in none)


def test_the_digest_of_the_parameters_does_not_depend_on_the_tuning():
    """periodic_rows is a choice of kernel: it is a field of the tuning, which the digest does not cover, and the detection leaves
    the circuit's shape as it was"""
    assert "periodic_rows" in tuning_default().as_dict()
    before = shape_digest_custom(F(5, "repeat"))
    assert shape_periodic_custom(F(5, "repeat"))[0] is not None
    assert shape_digest_custom(F(5, "repeat")) == before == shape_digest_custom(F(5, "loop"))
