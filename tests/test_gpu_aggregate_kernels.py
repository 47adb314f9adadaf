"""GPU: the two kernels of the relaxed-relaxed fold (vdf_cross_term_relaxed, vdf_fold_relaxed; include/vdf_hip.h), exact against
Python big integers (tests/aggregate_spec.py) in both fields.

Sizes: 1, one short of / exactly / one past a wavefront (63, 64, 65) and a workgroup (255, 256, 257), and 1000 (four workgroups, the
last one partly filled).  Vectors: random canonical elements salted with 0, 1 and m - 1; u1, u2 and r each over {0, 1, m - 1,
random}.  Then the two identities the header states (u2 = 1 gives vdf_cross_term's bytes; E2 = 0 gives the bytes of the vdf_axpy
sequence a step uses), n = 0, and the refusals."""
import numpy as np
import pytest

import aggregate_spec as ag
from oracle import pasta as o
from util import dev, host, ints, mont, unmont
from vdf_amd.hip import VdfError

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
FIELDS = ((o.FIELD_FP, o.P), (o.FIELD_FQ, o.Q))
BAD_ARG = 1
NULL = "null argument"
ON_HOST = "scalar operands of fused calls live in host memory"
ON_DEVICE = "vector operands of fused calls live in device memory"


def vectors(seed, k, n, m):
    """k vectors of n canonical elements: random, with 0, 1 and m - 1 salted in at fixed places (as far as n allows)"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(k):
        v = [int.from_bytes(rng.bytes(32), "little") % m for _ in range(n)]
        for pos, val in ((j % n, 0), ((j + 3) % n, 1), ((2 * j + 7) % n, m - 1)):
            v[pos] = val
        out.append(v)
    return out


def scalars(seed, m):
    return (0, 1, m - 1, o.rand_fe(seed, 0, m))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("field,m", FIELDS)
def test_cross_term_relaxed_is_exact(ctx, field, m, n):
    vs = vectors(100 + n, 6, n, m)
    d = [dev(mont(v, m)) for v in vs]
    T = dev(np.zeros((n, 4), dtype="<u8"))
    for u1 in scalars(1, m):
        for u2 in scalars(2, m):
            ctx.cross_term_relaxed(field, d[0], d[1], d[2], mont([u1], m), d[3], d[4], d[5], mont([u2], m), n, T)
            ctx.sync()
            assert unmont(host(T), m) == ag.cross_term_relaxed(vs[0], vs[1], vs[2], u1, vs[3], vs[4], vs[5], u2, m), (u1, u2)
    for x, v in zip(d, vs):
        assert unmont(host(x), m) == v                                     # the inputs are left as they were


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("field,m", FIELDS)
def test_fold_relaxed_is_exact(ctx, field, m, n):
    vs = vectors(200 + n, 9, n, m)
    ro = [dev(mont(v, m)) for v in vs[4:]]
    for r in scalars(3, m):
        acc = [dev(mont(v, m)) for v in vs[:4]]
        ctx.fold_relaxed(field, mont([r], m), n, acc[0], acc[1], acc[2], acc[3], ro[0], ro[1], ro[2], ro[3], ro[4])
        ctx.sync()
        want = ag.fold_relaxed(r, *vs[:4], *vs[4:8], vs[8], m)
        for k in range(4):
            assert unmont(host(acc[k]), m) == want[k], (r, k)
    for x, v in zip(ro, vs[4:]):
        assert unmont(host(x), m) == v


@pytest.mark.parametrize("field,m", FIELDS)
def test_fresh_second_instance_gives_the_existing_kernels_bytes(ctx, field, m):
    """u2 = 1: vdf_cross_term's T byte for byte.  E2 = 0 and a strict second instance: the fold is the vdf_axpy sequence of a step
    (A z, B z, C z and E each += r times the fresh vector / T), byte for byte."""
    n = 777
    vs = vectors(300, 8, n, m)
    d = [dev(mont(v, m)) for v in vs]
    u1, one, r = mont([o.rand_fe(4, 0, m)], m), mont([1], m), mont([o.rand_fe(5, 0, m) >> 130], m)      # (r: 128 bits at most, as a challenge)
    T0, T1 = dev(np.zeros((n, 4), dtype="<u8")), dev(np.full((n, 4), 7, dtype="<u8"))
    ctx.cross_term(field, d[0], d[1], d[2], d[3], d[4], d[5], u1, n, T0)
    ctx.cross_term_relaxed(field, d[0], d[1], d[2], u1, d[3], d[4], d[5], one, n, T1)
    ctx.sync()
    assert np.array_equal(host(T0), host(T1))
    zero = dev(np.zeros((n, 4), dtype="<u8"))
    a = [dev(mont(v, m)) for v in (vs[0], vs[1], vs[2], vs[6])]
    b = [dev(mont(v, m)) for v in (vs[0], vs[1], vs[2], vs[6])]
    ctx.fold_relaxed(field, r, n, a[0], a[1], a[2], a[3], d[3], d[4], d[5], zero, T0)
    for acc, add in zip(b, (d[3], d[4], d[5], T0)):
        ctx.axpy(field, acc, r, add, n, acc)
    ctx.sync()
    for x, y in zip(a, b):
        assert np.array_equal(host(x), host(y))


def test_n_zero_launches_nothing(ctx):
    one = mont([1], o.Q)
    ctx.set_kernel_timing(True)
    try:
        ctx.kernel_events()
        ctx.cross_term_relaxed(o.FIELD_FQ, None, None, None, one, None, None, None, one, 0, None)
        ctx.fold_relaxed(o.FIELD_FQ, one, 0, None, None, None, None, None, None, None, None, None)
        ctx.sync()
        assert ctx.kernel_events() == []
    finally:
        ctx.set_kernel_timing(False)


def refused(ctx, call, want):
    ctx.kernel_events()
    try:
        call()
    except VdfError as err:
        assert (err.code, str(err)) == (BAD_ARG, f"vdf_hip error {BAD_ARG}: {want}")
    else:
        pytest.fail("the call was not refused")
    assert ctx.kernel_events() == []


def test_refusals(ctx):
    """Per call and operand: NULL, a host array where a vector belongs, a device element where a host scalar belongs; an unknown
    field.  Nothing is launched and no vector changes."""
    n, m, f = 5, o.Q, o.FIELD_FQ
    vs = vectors(400, 9, n, m)
    d = [dev(mont(v, m)) for v in vs]
    one, one_dev, on_host = mont([1], m), dev(mont([1], m)), mont(vs[0], m)
    ctx.set_kernel_timing(True)
    try:
        cross = lambda p: ctx.cross_term_relaxed(f, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], n, p[8])
        good = [d[0], d[1], d[2], one, d[3], d[4], d[5], one, d[6]]
        for k in range(9):
            scalar = k in (3, 7)
            for bad, want in ((None, NULL), (one_dev if scalar else on_host, ON_HOST if scalar else ON_DEVICE)):
                p = list(good)
                p[k] = bad
                refused(ctx, lambda: cross(p), want)
        fold = lambda p: ctx.fold_relaxed(f, p[0], n, *p[1:])
        good = [one] + d[:9]
        for k in range(10):
            for bad, want in ((None, NULL), (one_dev if k == 0 else on_host, ON_HOST if k == 0 else ON_DEVICE)):
                p = list(good)
                p[k] = bad
                refused(ctx, lambda: fold(p), want)
        refused(ctx, lambda: ctx.cross_term_relaxed(7, d[0], d[1], d[2], one, d[3], d[4], d[5], one, n, d[6]), "unknown field")
        refused(ctx, lambda: ctx.fold_relaxed(7, one, n, *d[:9]), "unknown field")
        ctx.sync()
        for x, v in zip(d, vs):
            assert ints(host(x)) == ints(mont(v, m))
    finally:
        ctx.set_kernel_timing(False)
