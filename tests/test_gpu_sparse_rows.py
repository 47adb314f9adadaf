"""GPU: the seven kernels that walk the CSR rows of a vdf_shape (vdf_amd/csrc/vecops.hip) -- k_spmv, k_spmv_long, k_nifs_cross,
k_nifs_cross_w<4>, k_nifs_cross_w<8>, k_nifs_cross_f, k_relaxed_residual_batch -- against big-integer references, on shapes whose
row lengths, long-row positions, coefficients and columns are chosen (tests/sparse_rows_spec.py; its census is asserted by
tests/test_sparse_rows_host.py), in every lane count, with the long rows inside the launch and ahead of it, and on row ranges
that begin and end at the edges of groups, wavefronts and workgroups.

How every output is checked: every output buffer starts as all-ones garbage; the rows a call selects must equal the reference
exactly; the rows it does not select must still hold the garbage.  Every cross-term case asserts the labels of the timed launches
(vdf_ctx_kernel_events), so no case passes by running another kernel than the one it names.

What the suite showed these kernels before.  The direct tests ran eight lanes per row only.  One lane and four lanes per row
ran under test_hip_tuning_changes_scheduling_only alone, which compares proof bytes of the built-in reference circuit at t = 80;
the (matrix, row length) pairs of that circuit's two shapes are all it could show them (tests/test_sparse_rows_host.py keeps
this table current):

    side 0, 10820 rows: A 1-2,4-61,126,128,251,254,259,382; B 1-61,126,129,250-251; C 0-4,127,130,382
    side 1, 10049 rows: A 1-2,4-61,126,128,251,254,259,382; B 1-61,126,130,250-253; C 0-3,127,130,382

No row with an empty A or B, none with A at 3, none with C between 5 and 126, no row range on a shape with long rows, and the
rows there are not chosen against each other: which lengths meet in one row is whatever the circuit has.

The INSIDE side of the 2^15 boundary runs on a shape of its own ("boundary", 33537 rows): between the long rows that the large
shape must have at 256 and at 32767 lie 32510 rows, fewer than 2^15."""
import contextlib
import ctypes

import numpy as np
import pytest

from oracle import pasta as o
import sparse_rows_spec as S
from util import dev, host, mont
from vdf_amd import hip
from vdf_amd.hip import VdfError

pytestmark = pytest.mark.gpu
FIELDS = [o.FIELD_FP, o.FIELD_FQ]
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
ALL, INSIDE, OUTSIDE = S.ROWS_ALL, S.ROWS_INSIDE, S.ROWS_OUTSIDE
# (nifs_lanes, nifs_fused, the cross-term kernel of a call over the whole small shape): one configuration per kernel
PER_KERNEL = [(0, 1, "k_nifs_cross_f"), (8, 0, "k_nifs_cross_w8"), (4, 0, "k_nifs_cross_w4"), (1, 0, "k_nifs_cross")]


@contextlib.contextmanager
def tuned(**fields):
    """The tuning is global to the process: set for the block, restored after it whatever happens."""
    base = hip.tuning_get()
    try:
        hip.tuning_set(**fields)
        yield
    finally:
        hip.lib.vdf_hip_tuning_set(ctypes.byref(base))


@pytest.fixture(autouse=True)
def timed(ctx):
    ctx.set_kernel_timing(True)
    ctx.kernel_events()
    yield
    ctx.kernel_events()
    ctx.set_kernel_timing(False)


def garbage(n, count=1):
    return [dev(np.full((n, 4), ONES, dtype="<u8")) for _ in range(count)]


class Case:
    """A shape on the device, the operands of a cross term over it and the reference's results; never changed after it is made."""

    def __init__(self, ctx, name, field):
        self.field, self.m = field, o.modulus(field)
        m = self.m
        self.mats, self.cen = S.make_shape(name, field)
        self.n, self.ncols = self.cen["num_cons"], self.cen["num_cols"]
        self.shape = ctx.shape_create(field, self.n, self.ncols, self.mats)
        rng = np.random.default_rng([31, field, self.n])
        self.z = S.rand_ints(rng, m, self.ncols)
        self.zl = mont(self.z, m)
        self.dz = dev(self.zl)
        self.prods = S.products(self.mats, m, self.n, self.z)
        self.abc1 = [S.rand_ints(rng, m, self.n) for _ in range(3)]
        self.d1 = [dev(mont(x, m)) for x in self.abc1]
        self.u1 = S.rand_ints(rng, m, 1)[0]
        self.exp3 = [mont(p, m) for p in self.prods]
        self.exp4 = self.expected(self.u1)

    def expected(self, u1, prods=None):
        """[A z2, B z2, C z2, T] as Montgomery limbs"""
        prods = self.prods if prods is None else prods
        three = self.exp3 if prods is self.prods else [mont(p, self.m) for p in prods]
        return three + [mont(S.cross_term(*self.abc1, *prods, u1, self.m), self.m)]

    def mask(self, part, begin, count):
        inside = np.zeros(self.n, dtype=bool)
        inside[begin:begin + count] = True
        return np.ones(self.n, dtype=bool) if part == ALL else (inside if part == INSIDE else ~inside)


@pytest.fixture(scope="module")
def world(ctx):
    cache = {}

    def get(name, field):
        if (name, field) not in cache:
            cache[name, field] = Case(ctx, name, field)
        return cache[name, field]
    yield get
    for c in cache.values():
        c.shape.free()


def cross(ctx, c, part, begin=0, count=0, bufs=None, u1=None, dz=None):
    """One call on `bufs` (fresh garbage by default): (bufs, labels of its timed launches)"""
    bufs = garbage(c.n, 4) if bufs is None else bufs
    u1l = mont([c.u1 if u1 is None else u1], c.m)
    dz = c.dz if dz is None else dz
    ctx.kernel_events()
    if part == ALL:
        ctx.nifs_cross_term(c.shape, dz, *c.d1, u1l, *bufs)
    else:
        ctx.nifs_cross_term_rows(c.shape, begin, count, part, dz, *c.d1, u1l, *bufs)
    ctx.sync()
    return bufs, [e[0] for e in ctx.kernel_events()]


def check(c, bufs, exp4, written, what=""):
    """Exact on the rows `written` (bool[n]), garbage everywhere else"""
    for name, got, e in zip(("Az2", "Bz2", "Cz2", "T"), bufs, exp4):
        g = host(got).reshape(-1, 4)
        bad = np.nonzero(written & (g != e).any(axis=1))[0]
        assert bad.size == 0, (what, name, "differs from the reference at rows", bad[:8].tolist(), int(bad.size))
        dirty = np.nonzero(~written & (g != ONES).any(axis=1))[0]
        assert dirty.size == 0, (what, name, "written outside the selection at rows", dirty[:8].tolist(), int(dirty.size))


# ---- vdf_spmv3: k_spmv_long, then k_spmv per matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["small", "large"])
def test_spmv3(ctx, world, name, field, where):
    c = world(name, field)
    outs = [np.full((c.n, 4), ONES, dtype="<u8") for _ in range(3)] if where == "host" else garbage(c.n, 3)
    ctx.kernel_events()
    ctx.spmv3(c.shape, c.zl if where == "host" else c.dz, *outs)
    ctx.sync()
    assert [e[0] for e in ctx.kernel_events()] == ["k_spmv_long"]          # (k_spmv itself is not a timed launch)
    for k, (got, e) in enumerate(zip(outs, c.exp3)):
        g = got if where == "host" else host(got).reshape(-1, 4)
        bad = np.nonzero((g != e).any(axis=1))[0]
        assert bad.size == 0, ("ABC"[k], bad[:8].tolist(), int(bad.size))


# ---- vdf_nifs_cross_term over the whole shape ---------------------------------------------------------------------------------
SMALL_ALL = {(0, 1): ["k_nifs_cross_f"], (8, 1): ["k_nifs_cross_f"],
             (0, 0): ["k_spmv_long", "k_nifs_cross_w8"], (8, 0): ["k_spmv_long", "k_nifs_cross_w8"],
             (4, 1): ["k_spmv_long", "k_nifs_cross_w4"], (4, 0): ["k_spmv_long", "k_nifs_cross_w4"],
             (1, 1): ["k_spmv_long", "k_nifs_cross"], (1, 0): ["k_spmv_long", "k_nifs_cross"]}


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("lanes", [0, 1, 4, 8])
@pytest.mark.parametrize("field", FIELDS)
def test_cross_term_whole_small_shape(ctx, world, field, lanes, fused):
    c = world("small", field)
    with tuned(nifs_lanes=lanes, nifs_fused=fused):
        bufs, labels = cross(ctx, c, ALL)
    assert labels == SMALL_ALL[lanes, fused] == S.expected_labels(ALL, 0, c.cen, lanes, fused)
    check(c, bufs, c.exp4, c.mask(ALL, 0, 0))


LARGE_ALL = {(0, 1): ["k_spmv_long", "k_nifs_cross"], (0, 0): ["k_spmv_long", "k_nifs_cross"],
             (4, 1): ["k_spmv_long", "k_nifs_cross_w4"], (4, 0): ["k_spmv_long", "k_nifs_cross_w4"],
             (8, 1): ["k_nifs_cross_f"], (8, 0): ["k_spmv_long", "k_nifs_cross_w8"]}


@pytest.mark.parametrize("lanes", [0, 4, 8])
@pytest.mark.parametrize("field", FIELDS)
def test_cross_term_whole_large_shape(ctx, world, field, lanes):
    """Above 2^15 rows the default route is k_spmv_long followed by the lane-per-row kernel."""
    c = world("large", field)
    for fused in (1, 0):
        with tuned(nifs_lanes=lanes, nifs_fused=fused):
            bufs, labels = cross(ctx, c, ALL)
        assert labels == LARGE_ALL[lanes, fused] == S.expected_labels(ALL, 0, c.cen, lanes, fused), (lanes, fused)
        check(c, bufs, c.exp4, c.mask(ALL, 0, 0), (lanes, fused))


# ---- vdf_nifs_cross_term_rows: INSIDE and OUTSIDE of every range, in every lane mode ----------------------------------------------
@pytest.mark.parametrize("lanes", [0, 1, 4, 8])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["small", "large"])
def test_cross_term_rows(ctx, world, name, field, lanes):
    """Per range and nifs_fused mode: INSIDE on garbage (the range exact, the rest garbage), then OUTSIDE on the same buffers (every
    row exact); and OUTSIDE alone on garbage (the range still garbage, the rest exact)."""
    c = world(name, field)
    everything = c.mask(ALL, 0, 0)
    for begin, count in S.row_ranges(c.cen):
        for fused in (1, 0):
            what = (begin, count, lanes, fused)
            with tuned(nifs_lanes=lanes, nifs_fused=fused):
                bufs, labels = cross(ctx, c, INSIDE, begin, count)
                assert labels == S.expected_labels(INSIDE, count, c.cen, lanes, fused), what
                assert not any(x in labels for x in ("k_spmv_long", "k_nifs_cross_f")), what
                check(c, bufs, c.exp4, c.mask(INSIDE, begin, count), what + ("inside",))
                _, labels = cross(ctx, c, OUTSIDE, begin, count, bufs=bufs)
                want = S.expected_labels(OUTSIDE, count, c.cen, lanes, fused)
                assert labels == want and ("k_spmv_long" in labels) == ("k_nifs_cross_f" not in labels), what
                check(c, bufs, c.exp4, everything, what + ("inside, then outside",))
                alone, labels = cross(ctx, c, OUTSIDE, begin, count)
                assert labels == want, what
                check(c, alone, c.exp4, c.mask(OUTSIDE, begin, count), what + ("outside",))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["small", "large"])
def test_cross_term_rows_refusals(ctx, world, name, field):
    """A range that holds a long row and a range beyond the shape are refused, and nothing is written or launched."""
    c = world(name, field)
    n, nothing = c.n, np.zeros(c.n, dtype=bool)
    with_long = [(30, 3), (0, 1), (n - 1, 1), (33, 31), (65, 191), (1, n - 1)]
    beyond = [(n, 1), (n + 1, 0), (n - 5, 6), (1, n)]
    bufs = garbage(n, 4)
    for part in (INSIDE, OUTSIDE):
        for fused in (1, 0):
            for k, (begin, count) in enumerate(with_long + beyond):
                with tuned(nifs_fused=fused):
                    with pytest.raises(VdfError) as e:
                        cross(ctx, c, part, begin, count, bufs=bufs)
                assert e.value.code == (1 if k < len(with_long) else 2), (part, begin, count)     # VDF_ERR_BAD_ARG / VDF_ERR_BAD_LENGTH
                assert ctx.kernel_events() == []
    ctx.sync()
    check(c, bufs, c.exp4, nothing)


# ---- the boundary at 2^15 rows of a launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_outside_at_the_2_15_boundary(ctx, world, field):
    """33025 rows at the default tuning: with 257 rows left out the launch has 2^15 rows and is the fused one of eight lanes; with
    256 left out it has one row more and is k_spmv_long followed by the lane-per-row kernel."""
    c = world("large", field)
    assert c.n == S.LANE_LIMIT + 257
    with tuned(nifs_lanes=0, nifs_fused=1):
        for count, want in ((257, ["k_nifs_cross_f"]), (256, ["k_spmv_long", "k_nifs_cross"])):
            for begin in (1000, 32766 - count + 1):
                bufs, labels = cross(ctx, c, OUTSIDE, begin, count)
                assert labels == want, (begin, count)
                check(c, bufs, c.exp4, c.mask(OUTSIDE, begin, count), (begin, count))


@pytest.mark.parametrize("field", FIELDS)
def test_inside_at_the_2_15_boundary(ctx, world, field):
    """A range of 2^15 short rows runs eight lanes per row, a range of one more the lane-per-row kernel (default tuning)."""
    c = world("boundary", field)
    begin, length = max(c.cen["short_runs"], key=lambda r: r[1])
    assert length > S.LANE_LIMIT
    with tuned(nifs_lanes=0, nifs_fused=1):
        for count, want in ((S.LANE_LIMIT + 1, ["k_nifs_cross"]), (S.LANE_LIMIT, ["k_nifs_cross_w8"])):
            bufs, labels = cross(ctx, c, INSIDE, begin, count)
            assert labels == want, count
            check(c, bufs, c.exp4, c.mask(INSIDE, begin, count), count)


# ---- u1 at its edges; z2[0], which the kernels load for absent slots ------------------------------------------------------------
@pytest.mark.parametrize("lanes,fused,kernel", PER_KERNEL)
@pytest.mark.parametrize("field", FIELDS)
def test_u1_edges(ctx, world, field, lanes, fused, kernel):
    c = world("small", field)
    for u1 in (0, 1, c.m - 1):
        with tuned(nifs_lanes=lanes, nifs_fused=fused):
            bufs, labels = cross(ctx, c, ALL, u1=u1)
        assert labels[-1] == kernel and labels == S.expected_labels(ALL, 0, c.cen, lanes, fused)
        check(c, bufs, c.expected(u1), c.mask(ALL, 0, 0), u1)


@pytest.mark.parametrize("field", FIELDS)
def test_z2_element_0_never_contributes_to_absent_slots(ctx, world, field):
    """Where a row has fewer entries than a kernel prefetches, the kernel loads z2[0] in their place.  Two z2 that differ in element 0
    alone: the rows that do not name column 0 have the same products in both, and every kernel gives exactly those."""
    c = world("small", field)
    z = list(c.z)
    z[0] = c.m - 1
    assert c.z[0] not in (0, z[0])
    prods = S.products(c.mats, c.m, c.n, z)
    names0 = np.zeros(c.n, dtype=bool)
    for rows, cols, _ in c.mats:
        names0[rows[cols == 0]] = True
    free = np.nonzero(~names0)[0]
    assert free.size >= c.cen["short_rows_with_an_absent_slot_and_no_column_0"] > 100
    assert all(prods[k][r] == c.prods[k][r] for k in range(3) for r in free.tolist())
    assert any(prods[k][r] != c.prods[k][r] for k in range(3) for r in np.nonzero(names0)[0].tolist())
    exp4, dz = c.expected(c.u1, prods), dev(mont(z, c.m))
    for lanes, fused, kernel in PER_KERNEL:
        with tuned(nifs_lanes=lanes, nifs_fused=fused):
            bufs, labels = cross(ctx, c, ALL, dz=dz)
        assert labels[-1] == kernel
        check(c, bufs, exp4, c.mask(ALL, 0, 0), kernel)
        for got, here, there in zip(bufs[:3], exp4, c.exp3):                # the rows free of column 0: as with the other z2
            assert np.array_equal(host(got).reshape(-1, 4)[free], there[free]) and np.array_equal(here[free], there[free])


# ---- vdf_relaxed_residual_batch -----------------------------------------------------------------------------------------------
RESIDUAL_MAX = 64
# (count, E: "null" = no array, "nones" = an array of NULLs, "all", "mixed"; a, b: where the cycles of rho and u begin)
RESIDUAL_CASES = [(1, "null", 0, 3), (1, "all", 1, 0), (1, "nones", 2, 2), (1, "all", 3, 1), (1, "null", 1, 1),
                  (2, "mixed", 2, 2), (2, "null", 0, 0), (2, "all", 1, 3), (2, "nones", 3, 0),
                  (64, "all", 0, 0), (64, "null", 1, 1), (64, "mixed", 2, 3), (64, "nones", 3, 2)]


class Instances:
    """64 instances over a case's shape: z, E, their products by the reference, the edge values of rho and u"""

    def __init__(self, c, count):
        m = c.m
        rng = np.random.default_rng([47, c.field, c.n])
        self.zs = [S.rand_ints(rng, m, c.ncols) for _ in range(count)]
        self.Es = [S.rand_ints(rng, m, c.n) for _ in range(count)]
        self.dzs = [dev(mont(z, m)) for z in self.zs]
        self.dEs = [dev(mont(E, m)) for E in self.Es]
        self.prods = [S.products(c.mats, m, c.n, z) for z in self.zs]
        self.rho_rand = [int.from_bytes(rng.bytes(16), "little") for _ in range(count)]
        self.u_rand = S.rand_ints(rng, m, count)

    def rho(self, q, a):
        return (0, 1, 2**128 - 1, self.rho_rand[q])[(q + a) % 4]

    def u(self, q, b, m):
        return (0, 1, m - 1, self.u_rand[q])[(q + q // 4 + b) % 4]


@pytest.fixture(scope="module")
def instances(world):
    cache = {}

    def get(name, field, count):
        if (name, field) not in cache:
            cache[name, field] = Instances(world(name, field), count)
        return cache[name, field]
    return get


def w128(vals):
    return np.array([[v & (2**64 - 1), v >> 64, 0, 0] for v in vals], dtype="<u8").reshape(-1, 4)


def residual_call(ctx, c, dzs, dEs, us, rhos, out):
    """dEs None: the E argument itself is NULL (the wrapper always passes an array)"""
    if dEs is not None:
        return ctx.relaxed_residual_batch(c.shape, dzs, dEs, mont(us, c.m), w128(rhos), out)
    count = len(dzs)
    z = (ctypes.c_void_p * count)(*[t.data_ptr() for t in dzs])
    u, r = mont(us, c.m), w128(rhos)
    ctx._check(hip.lib.vdf_relaxed_residual_batch(ctx.handle, c.shape.handle, count, z, None, u.ctypes.data, r.ctypes.data, out.data_ptr()))


def run_residual(ctx, c, inst, count, emode, a, b):
    m = c.m
    us = [inst.u(q, b, m) for q in range(count)]
    rhos = [inst.rho(q, a) for q in range(count)]
    given = [emode == "all" or (emode == "mixed" and q % 3 != 1) for q in range(count)]
    dEs = None if emode == "null" else [inst.dEs[q] if given[q] else None for q in range(count)]
    Es = None if emode == "null" else [inst.Es[q] if given[q] else None for q in range(count)]
    (out,) = garbage(c.n)
    ctx.kernel_events()
    residual_call(ctx, c, inst.dzs[:count], dEs, us, rhos, out)
    ctx.sync()
    assert [e[0] for e in ctx.kernel_events()] == ["k_relaxed_residual_batch"[:23]]      # (an event keeps 23 characters of its label)
    want = S.residual(c.mats, m, inst.zs[:count], Es, us, rhos, num_cons=c.n, prods=inst.prods[:count])
    g = host(out).reshape(-1, 4)
    bad = np.nonzero((g != mont(want, m)).any(axis=1))[0]
    assert bad.size == 0, (bad[:8].tolist(), int(bad.size))
    return want, us, rhos


@pytest.mark.parametrize("count,emode,a,b", RESIDUAL_CASES)
@pytest.mark.parametrize("field", FIELDS)
def test_residual_batch_small_shape(ctx, world, instances, field, count, emode, a, b):
    c = world("small", field)
    inst = instances("small", field, RESIDUAL_MAX)
    want, us, rhos = run_residual(ctx, c, inst, count, emode, a, b)
    if count == 1 and rhos[0] == 0:
        assert not any(want)                                                 # the garbage is overwritten with zeros
    if count == 64:                                                          # every pair of a rho edge and a u edge is in the batch
        rk = lambda r: {0: 0, 1: 1, 2**128 - 1: 2}.get(r, 3)
        uk = lambda u: {0: 0, 1: 1, c.m - 1: 2}.get(u, 3)
        kinds = {(rk(r), uk(u)) for r, u in zip(rhos, us)}
        assert len(kinds) == 16


@pytest.mark.parametrize("field", FIELDS)
def test_residual_batch_large_shape(ctx, world, instances, field):
    c = world("large", field)
    run_residual(ctx, c, instances("large", field, 2), 2, "mixed", 2, 2)


@pytest.mark.parametrize("field", FIELDS)
def test_residual_batch_refuses_no_instance_and_65(ctx, world, instances, field):
    c = world("small", field)
    inst = instances("small", field, RESIDUAL_MAX)
    (out,) = garbage(c.n)
    for count in (0, 65):
        dzs = [inst.dzs[q % RESIDUAL_MAX] for q in range(count)]
        for dEs in ([None] * count, [inst.dEs[q % RESIDUAL_MAX] for q in range(count)]):
            with pytest.raises(VdfError) as e:
                ctx.relaxed_residual_batch(c.shape, dzs, dEs, mont([1] * max(count, 1), c.m), w128([1] * max(count, 1)), out)
            assert e.value.code == 1
            assert ctx.kernel_events() == []
    ctx.sync()
    assert (host(out) == ONES).all()
