"""tests/prim_spec.py itself -- the Python-integer reference of the device primitives and its case generators -- and the
runner tools/ubench/prim_check on the host instantiation of fe.cuh / ec.cuh (`--host`: no device).  Every comparison is an
equality; every bound is recomputed from the modulus."""
import random

import pytest

import prim_spec as s
from oracle import pasta as o

FIELDS = pytest.mark.parametrize("F", s.FIELDS, ids=repr)


@FIELDS
def test_redc_is_multiplication_mod_m(F):
    """redc composed with to_mont / from_mont is multiplication mod m, on edges and 10^4 random values"""
    m = F.m
    rng = random.Random(41 + F.fid)
    edges = [0, 1, 2, m - 2, m - 1, (m - 1) // 2, (m + 1) // 2, F.c, F.one, F.r2, 1 << 253, (1 << 254) - 1]
    pairs = [(a, b) for a in edges for b in edges] + [(rng.randrange(m), rng.randrange(m)) for _ in range(10000)]
    assert F.nminv * m % s.R == s.R - 1 and F.nminv & 0xFFFFFFFF == 0xFFFFFFFF        # fe.cuh: the quotient digit is the negated low limb
    for a, b in pairs:
        t = s.redc(F, o.to_mont(a, m) * o.to_mont(b, m))
        assert t < 2 * m and o.from_mont(t, m) == a * b % m
        assert s.fe_mul_inl(F, o.to_mont(a, m), o.to_mont(b, m)) == o.to_mont(a * b, m)
    assert s.fe_from_small(F, 12345) == o.to_mont(12345, m) and s.fe_to_mont(F, s.fe_from_mont(F, 7)) == 7
    assert s.fe_inv(F, 0) == 0 and s.fe_mul_inl(F, s.fe_inv(F, F.r2), F.r2) == F.one


@FIELDS
def test_slack_invariant_closes(F):
    """eps as the issue defines it, and the per-coordinate invariant of both lazy additions in exact interval arithmetic"""
    assert F.eps == -((-F.m * (F.m - (1 << 254))) // (1 << 254)) and 1 << 125 < F.eps < 1 << 126
    assert s.closes(F)
    assert 2 * F.m + 9 * F.eps < 1 << 256 and 3 * F.m + 2 * F.eps + 2 * 9 * F.eps < 1 << 256          # fe_mul2_lazy's stated precondition


@FIELDS
def test_field_case_generators_keep_their_promises(F):
    m = F.m
    for op, (arity, bound, pre) in s.FIELD_OPS.items():
        cases = s.field_cases(F, op)
        assert 64 < len(cases) <= 8192 and len(cases) % 64 != 0, op               # full wavefronts and a partial one
        assert all(len(t) == arity for t in cases), op
        top = 3 * m if op == "fe_canon" else bound(F)
        assert all(0 <= v < top for t in cases for v in t), op
        if op not in ("fe_inv", "fe_is_canonical"):                                # all three ranges, as far as the contract reaches
            for lo, hi in ((0, m), (m, 2 * m), (2 * m, s.lazy_top(F))):
                if hi <= top:
                    assert sum(lo <= t[0] < hi for t in cases) > 100, (op, lo)
    # fe_mul2_lazy: both sides of the top-bit branch, and never a ninth word
    cases = s.field_cases(F, "fe_mul2_lazy")
    taken = sum(s.redc(F, a * b + c * d) >= 1 << 255 for a, b, c, d in cases)
    assert all(s.redc(F, a * b + c * d) < s.R for a, b, c, d in cases)
    assert taken >= len(cases) // 20 and len(cases) - taken >= len(cases) // 20
    # fe_sub_lazy: borrows and does not, and the precondition b <= a + 2m holds for every case
    cases = s.field_cases(F, "fe_sub_lazy")
    assert sum(a < b for a, b in cases) > 1000 and sum(a >= b for a, b in cases) > 1000
    assert all(0 <= s.fe_sub_lazy(F, a, b) < s.lazy_top(F) for a, b in cases)
    # the fast negations never see 0 (mod m)
    assert all(a % m for (a,) in s.field_cases(F, "fe_neg_lazy") + s.field_cases(F, "fe_neg_nz"))
    assert any(a >= 2 * m for (a,) in s.field_cases(F, "fe_neg_lazy")) and (3 * m - 1,) in s.field_cases(F, "fe_neg_lazy")


@FIELDS
def test_from_small_correction_branch_is_unreachable(F):
    """fe.cuh fe_from_small: r = (x mod 2^254) - q c, `plus m if that went negative`.  With R mod m = 2^254 - 3c one has
    x = k 2^254 - 3kc, q = k - 1 and r = 2^254 - (4k - 1) c > 0 for every 0 < k < 2^30 (c < 2^126): the correction is never taken
    inside the contract, so no generator can hit it; the cases cover k at both ends of the contract instead."""
    ks = [k for (k,) in s.field_cases(F, "fe_from_small")]
    assert all(0 <= k < 1 << 30 for k in ks) and {0, 1, (1 << 30) - 1} <= set(ks)
    assert F.one == (1 << 254) - 3 * F.c and (4 * (1 << 30) - 1) * F.c < 1 << 254
    assert not any(s.fe_from_small_went_negative(F, k) for k in ks)
    for k in ks[:64]:
        assert s.fe_from_small(F, k) == ((1 << 254) - (4 * k - 1) * F.c if k else 0)


@FIELDS
@pytest.mark.parametrize("lazy_add", (False, True), ids=("madd", "add"))
def test_lazy_addition_states(F, lazy_add):
    """the crafted accumulator states: what they must contain, and that the integer model of one step -- written from the
    formulas in ec.cuh's comment -- keeps every one of them inside the invariant and, for on-curve states, adds the points"""
    m = F.m
    cases = s.lazy_cases(F, lazy_add)
    slack2 = s.ADD_SLACK2 if lazy_add else s.MADD_SLACK2
    assert len(cases) > 128 and len(cases) % 64
    first_wave = [c.kind for c in cases[:64]]
    for kind in set(c.kind for c in cases):
        assert first_wave.count(kind) >= 2, kind                                 # several lanes of ONE wavefront, next to general additions
    want = {"general", "first", "small", "top"} | {"%s_P%d" % (k, p) for k in ("double", "cancel") for p in ((0, 1) if lazy_add else (0, 1, 2))}
    assert set(first_wave) == want
    on = [c for c in cases if c.have]
    assert any(c.acc[2] != F.one for c in on) and any(c.acc[2] == F.one for c in on)
    assert {c.flip for c in on} == {0, 1}
    for j, k in enumerate(slack2):
        if j in (0, 2):                                                           # v + 2m on a curve point: x and zz, by construction
            assert any(c.acc[j] >= 2 * m for c in on if c.on_curve), j
        assert any(c.acc[j] >= m for c in on if c.on_curve)
        assert any(c.acc[j] == s.limit(F, k) - 1 for c in on), j                  # the very top of the slack
    seen = set()
    for c in cases:
        assert all(v < m for v in c.b) and any(c.b), "b canonical and not the identity"
        if c.on_curve and c.stored is not None:
            assert o.on_curve(c.stored, F.curve) and s.xyzz_point(F, c.acc) == c.stored
        if c.have:
            assert s.inside(F, c.acc, slack2)
        acc, have, flip, Pn = (s.xyzz_add_lazy if lazy_add else s.xyzz_madd_lazy)(F, c.acc, c.have, c.flip, c.b)
        if have:
            assert s.inside(F, acc, slack2), c.kind
        if c.kind.startswith(("double", "cancel")):
            assert Pn in (0, m, 2 * m) and have == c.kind.startswith("double")
            seen.add((c.kind[:6], Pn // m, c.flip))
        if c.on_curve:
            res = s.xyzz_lazy_resolve(F, acc, have, flip)
            assert s.xyzz_point(F, res) == s.lazy_expected_point(F, c), c.kind
    assert seen == {(k, p, f) for k in ("double", "cancel") for p in ((0, 1) if lazy_add else (0, 1, 2)) for f in (0, 1)}


def _host_jobs(F):
    """every host-capable job; the lazy operands reduced mod m (the host's lazy operations are the canonical ones)"""
    m = F.m
    jobs, checks = [], []
    for op in list(s.FIELD_OPS) + ["fe_from_small"]:
        cases = s.field_cases(F, op)
        lazy = op in ("fe_mul_lazy", "fe_sqr_lazy", "fe_mul2_lazy", "fe_sub_lazy", "fe_neg_lazy", "fe_neg_nz", "fe_canon")
        rows = [tuple(v % m for v in t) for t in cases] if lazy else cases
        model = s.FIELD_MODEL[op]
        jobs.append((F, op, rows))
        checks.append([(model(F, *t) % m if lazy else model(F, *t),) for t in rows])
    cases = s.lazy_cases(F, False)
    for c in cases:
        c.acc = tuple(v % m for v in c.acc)
    jobs.append((F, "xyzz_madd_lazy", s.lazy_rows(cases)))
    checks.append([tuple(v % m if k not in (4, 5) else v for k, v in enumerate(s.lazy_model_row(F, False, c))) for c in cases])
    return jobs, checks


@FIELDS
def test_runner_on_the_host(F):
    """prim_check --host (build: make -C vdf_amd/csrc): the portable branches of fe.cuh and the group law of ec.cuh, one child"""
    jobs, checks = _host_jobs(F)
    group = [(op,) + s.group_cases(F, op) for op in s.GROUP_OPS]
    jobs += [(F, op, rows) for op, rows, _ in group]
    res = s.run_jobs(jobs, host=True)
    for (_, op, rows), got, want in zip(jobs, res, checks):
        bad = [i for i in range(len(rows)) if got[i] != want[i]]
        assert not bad, "%s %s: %d of %d differ, first operands %s" % (F, op, len(bad), len(rows), [hex(v) for v in rows[bad[0]]])
    for (op, rows, exp), got in zip(group, res[len(checks):]):
        s.check_group(F, op, rows, exp, got)
