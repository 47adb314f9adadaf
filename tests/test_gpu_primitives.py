"""The device primitives of fe.cuh, ec.cuh and ecq.cuh, in both fields, against tests/prim_spec.py (plain Python integers)
and oracle/pasta.py (the affine group law).  tools/ubench/prim_check applies each operation to the generated operands, one
lane (or one quad) per case, and returns the raw words; nothing is compared on the device, and every comparison here is an
equality -- of 256-bit integers for the field operations and the lazy additions, of group elements for the canonical law.
One child process per test."""
import pytest

import prim_spec as s

pytestmark = pytest.mark.gpu
FIELDS = pytest.mark.parametrize("F", s.FIELDS, ids=repr)


def _first_bad(F, op, rows, got, want):
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    assert not bad, "%s %s: %d of %d cases differ; first: operands %s -> got %s, want %s" % (
        F, op, len(bad), len(rows), [hex(v) for v in rows[bad[0]]], [hex(v) for v in got[bad[0]]], [hex(v) for v in want[bad[0]]])


@FIELDS
def test_field_operations_bit_for_bit(F):
    """every field operation on the edge list crossed with itself and 4,096 random operands from [0, m), [m, 2m) and
    [2m, 2m + 9 eps) -- as far as the operation's contract reaches -- against the integer semantics, bit for bit: the lazy
    products as redc(T) itself, fe_mul2_lazy on both sides of its top-bit branch, fe_sub_lazy with and without borrow,
    fe_neg_lazy up to 3m - 1 (and on the multiples of m, where 3m - a is exact as well)"""
    ops = list(s.FIELD_OPS) + ["fe_from_small"]
    jobs = [(F, op, s.field_cases(F, op)) for op in ops] + [(F, "fe_neg_lazy", s.NEG_LAZY_MULTIPLES(F))]
    res = s.run_jobs(jobs)
    for (_, op, rows), got in zip(jobs, res):
        model = s.FIELD_MODEL[op]
        _first_bad(F, op, rows, got, [(model(F, *t),) for t in rows])


def _lazy_addition(F, lazy_add):
    cases = s.lazy_cases(F, lazy_add)
    op = "xyzz_add_lazy" if lazy_add else "xyzz_madd_lazy"
    slack2 = s.ADD_SLACK2 if lazy_add else s.MADD_SLACK2
    rows = s.lazy_rows(cases)
    got, = s.run_jobs([(F, op, rows)])
    want = [s.lazy_model_row(F, lazy_add, c) for c in cases]
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    assert not bad, "%s %s: %d of %d cases differ from the integer model; kinds %s; first: lane %d (%s) got %s, want %s" % (
        F, op, len(bad), len(rows), sorted({cases[i].kind for i in bad}), bad[0], cases[bad[0]].kind,
        [hex(v) for v in got[bad[0]]], [hex(v) for v in want[bad[0]]])
    for c, g in zip(cases, got):
        if g[4]:
            assert s.inside(F, g[:4], slack2), (c.kind, [str(s.slack_in_eps(F, v)) for v in g[:4]])
        if c.on_curve:
            assert s.xyzz_point(F, g[6:]) == s.lazy_expected_point(F, c), c.kind


@FIELDS
def test_lazy_mixed_addition_on_crafted_states(F):
    """xyzz_madd_lazy + xyzz_lazy_resolve, side by side in one wavefront: general additions on accumulators with zz != 1 and
    zz = 1, representatives v / v + m / v + 2m, flip set and clear, coordinates at the top of their slack (off the curve: the
    integer model alone decides), the first addition, and b = +-acc with P' exactly 0, m and 2m.  Outputs bit-identical to the
    model, stored coordinates inside the invariant (eps, 9 eps, 4 eps, 4.5 eps), resolved point equal to oracle.pt_add."""
    _lazy_addition(F, False)


@FIELDS
def test_lazy_full_addition_on_crafted_states(F):
    """the same for xyzz_add_lazy (the lane-serial fix-up; invariant 4 eps throughout; P' = 2m is unreachable there, see
    tests/prim_spec.py), whose same-x branch falls back to the canonical law"""
    _lazy_addition(F, True)


@FIELDS
def test_canonical_group_law(F):
    """xyzz_madd (both INL), xyzz_add, xyzz_dbl, xyzz_dbl_affine, xyzz_to_jac, jac_to_xyzz, xyzz_to_affine, xyzz_mul_u64 against
    oracle.pt_add / pt_mul as group elements: general, P + P, P + (-P), the identity on either side and on both, zz = 1 and not"""
    group = [(op,) + s.group_cases(F, op) for op in s.GROUP_OPS]
    res = s.run_jobs([(F, op, rows) for op, rows, _ in group])
    for (op, rows, exp), got in zip(group, res):
        s.check_group(F, op, rows, exp, got)


@FIELDS
def test_quad_cooperative_law(F):
    """ecq.cuh: qpoint_add / qpoint_dbl / qpoint_neg with the 16 quads of a wavefront in different branches side by side
    (general, doubling, opposite, identity left / right / both; equal x through different zz), qpoint_load_lazy -> qpoint_store
    on lazy representatives (bit for bit), and qpoint_wave_sum over 16 points whose butterfly steps double, cancel and meet
    identities"""
    m = F.m
    quad = [(op,) + s.quad_cases(F, op) for op in ("qpoint_add", "qpoint_dbl", "qpoint_neg")]
    quad.append(("qpoint_wave_sum",) + s.wave_sum_cases(F))
    lrows, lout, linf = s.load_lazy_cases(F)
    res = s.run_jobs([(F, op, rows) for op, rows, _ in quad] + [(F, "qpoint_load_lazy", lrows)])
    for (op, rows, exp), got in zip(quad, res):
        for i, (g, e) in enumerate(zip(got, exp)):
            assert all(v < m for v in g[:4]) and g[4] == int(e is None), (op, i)
            assert s.xyzz_point(F, g[:4]) == e, "%s %s case %d" % (F, op, i)
            if e is None:
                assert g[:4] == (0, 0, 0, 0), (op, i)                    # qpoint_store writes the all-zero identity
    _first_bad(F, "qpoint_load_lazy", lrows, res[-1], [r + (f,) for r, f in zip(lout, linf)])
