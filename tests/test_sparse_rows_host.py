"""Host: the shapes, ranges and references that tests/test_gpu_sparse_rows.py runs the sparse-row kernels on
(tests/sparse_rows_spec.py).  The census keeps an edit of the builder from hollowing the GPU tests out; the big-integer
references are checked against the C restatement, an implementation that shares no code with them; and the row lengths of the
built-in circuit -- all that the proof-level tuning test ever showed the lane-per-row and four-lane kernels -- are tabulated
and compared with the record in the GPU test's docstring."""
import os

import numpy as np
import pytest

from oracle import pasta as o
import sparse_rows_spec as S
from util import mont

FIELDS = [o.FIELD_FP, o.FIELD_FQ]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", sorted(S.SHAPES))
def test_census_every_feature_is_present(name, field):
    mats, cen = S.make_shape(name, field)
    missing = [k for k in S.REQUIRED if not cen[k]]
    assert not missing, missing
    cfg = S.SHAPES[name]
    n = cfg["num_cons"]
    assert cen["num_cons"] == n and all(len(r) == len(c) == len(v) for r, c, v in mats)
    assert all(int(c.max()) < cfg["num_cols"] for _, c, _ in mats)
    assert n % 32 == n % 64 == n % 256 == 1
    assert set(cfg["extra_long"]) <= set(cen["long_rows"])
    assert cen["repeated_columns"] >= 4 and any(r not in cen["long_rows"] for _, r in cen["rows_built_with_a_repeat"]) \
        and any(r in cen["long_rows"] for _, r in cen["rows_built_with_a_repeat"])
    # the builder is deterministic
    again, _ = S.make_shape(name, field)
    assert all(np.array_equal(x, y) for a, b in zip(mats, again) for x, y in zip(a, b))
    # the ranges of the range calls: the starts and ends that must be among them
    rng = S.row_ranges(cen)
    starts, ends, longs = {b for b, _ in rng}, {b + c for b, c in rng}, set(cen["long_rows"])
    assert {0, n} <= starts & ends
    assert {(0, 0), (n // 2, 0), (n, 0)} <= set(rng)
    for base, who in ((96, "32"), (128, "64"), (512, "256")):
        assert {base - 1, base, base + 1} <= starts | ends, who
    assert any(b - 1 in longs and c for b, c in rng) and any(b + c in longs and c for b, c in rng)
    assert set(cen["short_runs"]) <= set(rng)
    if name == "small":
        assert n == 769 and 690 <= cfg["num_cols"] <= 710
    if name == "large":
        assert n == 33025 and {32767, 32768} <= longs
        # the OUTSIDE calls on both sides of 2^15 remaining rows need a short run of 257 rows
        assert cen["longest_short_run"] >= n - S.LANE_LIMIT
    if name == "boundary":
        assert cen["longest_short_run"] > S.LANE_LIMIT


def test_expected_labels_restate_the_selection():
    cen = {"num_cons": 769, "long_rows": [0]}
    f, w8, w4, w1, lg = "k_nifs_cross_f", "k_nifs_cross_w8", "k_nifs_cross_w4", "k_nifs_cross", "k_spmv_long"
    for lanes in (0, 8):
        assert S.expected_labels(S.ROWS_ALL, 0, cen, lanes, 1) == [f]
        assert S.expected_labels(S.ROWS_ALL, 0, cen, lanes, 0) == [lg, w8]
    for fused in (0, 1):
        assert S.expected_labels(S.ROWS_ALL, 0, cen, 4, fused) == [lg, w4]
        assert S.expected_labels(S.ROWS_ALL, 0, cen, 1, fused) == [lg, w1]
        assert S.expected_labels(S.ROWS_INSIDE, 5, cen, 0, fused) == [w8]
        assert S.expected_labels(S.ROWS_INSIDE, 0, cen, 0, fused) == []
    big = {"num_cons": 33025, "long_rows": [0]}
    assert S.expected_labels(S.ROWS_ALL, 0, big, 0, 1) == [lg, w1]
    assert S.expected_labels(S.ROWS_OUTSIDE, 257, big, 0, 1) == [f]
    assert S.expected_labels(S.ROWS_OUTSIDE, 256, big, 0, 1) == [lg, w1]
    assert S.expected_labels(S.ROWS_INSIDE, (1 << 15) + 1, big, 0, 1) == [w1]
    assert S.expected_labels(S.ROWS_INSIDE, 1 << 15, big, 0, 1) == [w8]


@pytest.mark.parametrize("field", FIELDS)
def test_two_independent_references_agree(cref, field):
    """Big integers against the C restatement's Montgomery arithmetic (oracle/pasta_ref.c), bit for bit."""
    m = o.modulus(field)
    mats, cen = S.make_shape("small", field)
    n, ncols = cen["num_cons"], cen["num_cols"]
    rng = np.random.default_rng(5 + field)
    z = S.rand_ints(rng, m, ncols)
    zl = mont(z, m)
    prods = S.products(mats, m, n, z)
    exp = []
    for (rows, cols, vals), p in zip(mats, prods):
        e = cref.fe_array(n)
        cref.lib().ref_spmv(field, cref.p(rows), cref.p(cols), cref.p(vals), len(rows), cref.p(zl), n, cref.p(e))
        assert np.array_equal(mont(p, m), e)
        exp.append(e)
    for u1 in (0, 1, m - 1, S.rand_ints(rng, m, 1)[0]):
        abc1 = [S.rand_ints(rng, m, n) for _ in range(3)]
        T = S.cross_term(*abc1, *prods, u1, m)
        eT = cref.fe_array(n)
        l1, lu = [mont(x, m) for x in abc1], mont([u1], m)                    # named: the pointers must outlive the call
        cref.lib().ref_cross_term(field, *(cref.p(x) for x in l1), *(cref.p(x) for x in exp), cref.p(lu), n, cref.p(eT))
        assert np.array_equal(mont(T, m), eT)
    # the residual restates its formula over the same products: one instance with rho = 1, u = 1 and no E is a b - c
    one = S.residual(mats, m, [z], None, [1], [1], prods=[prods])
    assert one == [(a * b - c) % m for a, b, c in zip(*prods)]
    assert one == S.residual(mats, m, [z], [None], [1], [1])
    E = S.rand_ints(rng, m, n)
    two = S.residual(mats, m, [z, z], [E, None], [1, 0], [3, 2**128 - 1], num_cons=n)
    assert two == [(3 * (x - e) + (2**128 - 1) * (x + c)) % m for x, e, c in zip(one, E, prods[2])]


def builtin_lengths_table(t=80):
    """The (matrix, row length) pairs of the built-in reference circuit's two shapes at t, one line per side"""
    from vdf_amd.nova import CIRCUIT_MINROOT_REFERENCE, shape_export
    lines = []
    for side in (0, 1):
        mats = shape_export(t, CIRCUIT_MINROOT_REFERENCE, side)
        n = 1 + max(int(r.max()) for r, _, _ in mats if len(r))
        tab = S.lengths_table(mats, n)
        lines.append(f"side {side}, {n} rows: " + "; ".join(f"{k} {_spans(v)}" for k, v in tab.items()))
    return lines


def _spans(v):
    out, i = [], 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and v[j + 1] == v[j] + 1:
            j += 1
        out.append(str(v[i]) if i == j else f"{v[i]}-{v[j]}")
        i = j + 1
    return ",".join(out)


def test_row_lengths_the_builtin_circuit_has_at_t_80():
    """test_hip_tuning_changes_scheduling_only forces nifs_lanes = 1 and 4 on this circuit only: what it showed those kernels is
    what this table holds.  The GPU test's docstring keeps the table; it must be the current one."""
    lines = builtin_lengths_table(80)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_sparse_rows.py")) as f:
        text = f.read()
    for line in lines:
        assert line in text, line
