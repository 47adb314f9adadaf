"""GPU: vdf_sparse_eval_multi (vdf_amd/csrc/vecops.hip k_sparse_eval_multi, k_sparse_eval_sum) -- every proof's M(r_x, r_y) in one
pass over a shape's rows -- equal to the big-integer statement of tests/sparse_eval_spec.py limb for limb, in both fields, on the
small shape of tests/sparse_rows_spec.py: 769 rows x 701 columns with every row length of LENGTHS, long rows at the fixed positions
and in the last row, and rows whose three matrices are all empty.

The vectors are random field vectors (the kernel does not know about eq tables); the counts go round the kernel's chunk of
instances per pass, whichever of 2 and 4 it was built with (1, 2, 3, 4, 5), and on to 16 and 64; the column map is the identity and a
split that leaves a gap; rho cycles through 0, 1, m - 1 and random values.  Unit vectors as eq_x isolate one row each -- row 0, a long
row, the last row, an all-empty row -- so that a slip at the grid's tail or in the long-row path cannot cancel against another
row.  The results always land in a host array that holds garbage before the call.  One case checks the call against the device's
own older sequence for the same point: vdf_pair_table -> vdf_spmv3_t -> vdf_reduce(DOT)."""
import ctypes

import numpy as np
import pytest

from oracle import pasta as o
import sparse_eval_spec as E
import sparse_rows_spec as S
from util import dev, host, ints, mont
from vdf_amd import hip
from vdf_amd.hip import VdfError

pytestmark = pytest.mark.gpu
FIELDS = [o.FIELD_FP, o.FIELD_FQ]
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX = 64                                          # VDF_SPARSE_EVAL_MAX
COUNTS = [1, 2, 3, 4, 5, 16, 64]                  # chunk - 1, chunk, chunk + 1 for a chunk of 2 and of 4; then many passes
# (col_split, col_hi_base, ny): the identity over the 701 columns; columns 600.. moved to 640.., a gap of 40 nothing reads
MAPS = {"identity": (701, 0, 701), "split": (600, 640, 741)}


class World:
    """The small shape on the device, 64 instances for each column map and the spec's value of every one; made once."""

    def __init__(self, ctx, field):
        self.field, self.m = field, o.modulus(field)
        m = self.m
        self.mats, self.cen = S.make_shape("small", field)
        self.n, self.ncols = self.cen["num_cons"], self.cen["num_cols"]
        assert (self.n, self.ncols) == (769, 701)
        self.shape = ctx.shape_create(field, self.n, self.ncols, self.mats)
        self.triples = [list(zip(r.tolist(), c.tolist(), S.unmont_unique(v, m))) for r, c, v in self.mats]
        rng = np.random.default_rng([53, field])
        self.ex = [S.rand_ints(rng, m, self.n) for _ in range(MAX)]
        self.dex = [dev(mont(x, m)) for x in self.ex]
        rand_rho = S.rand_ints(rng, m, MAX)
        self.rho = [(0, 1, m - 1, rand_rho[q])[(q + q // 4) % 4] for q in range(MAX)]
        self.ey, self.dey, self.want = {}, {}, {}
        for name, (split, base, ny) in MAPS.items():
            self.ey[name] = [S.rand_ints(rng, m, ny) for _ in range(MAX)]
            self.dey[name] = [dev(mont(y, m)) for y in self.ey[name]]
            self.want[name] = E.multi_eval(self.triples, m, self.ex, self.ey[name], self.rho, split, base)
        lens = S.row_lengths(self.mats, self.n)
        self.empty_row = int(np.nonzero((lens == 0).all(axis=1))[0][0])
        self.long_row = 255
        assert self.long_row in self.cen["long_rows"] and 0 in self.cen["long_rows"] and self.n - 1 in self.cen["long_rows"]

    def call(self, ctx, name, qs, dex=None, rho=None):
        split, base, _ = MAPS[name]
        out = np.full((len(qs), 4), ONES, dtype="<u8")                        # garbage before the call
        dex = [self.dex[q] for q in qs] if dex is None else dex
        rho = [self.rho[q] for q in qs] if rho is None else rho
        got = ctx.sparse_eval_multi(self.shape, dex, [self.dey[name][q] for q in qs], mont(rho, self.m), split, base, out=out)
        assert got is out
        return out


@pytest.fixture(scope="module")
def world(ctx):
    cache = {}

    def get(field):
        if field not in cache:
            cache[field] = World(ctx, field)
        return cache[field]
    yield get
    for w in cache.values():
        w.shape.free()


@pytest.fixture(autouse=True)
def timed(ctx):
    ctx.set_kernel_timing(True)
    ctx.kernel_events()
    yield
    ctx.kernel_events()
    ctx.set_kernel_timing(False)


def same(got, want_ints, m):
    bad = np.nonzero((got != mont(want_ints, m)).any(axis=1))[0]
    assert bad.size == 0, (bad[:8].tolist(), int(bad.size))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("field", FIELDS)
def test_equals_the_spec(ctx, world, field, name, count):
    w = world(field)
    qs = list(range(count))
    got = w.call(ctx, name, qs)
    assert [e[0] for e in ctx.kernel_events()] == ["k_sparse_eval_multi"]      # one timed evaluation (its two launches), nothing else
    same(got, w.want[name][:count], w.m)
    if count == MAX:
        kinds = {{0: 0, 1: 1, w.m - 1: 2}.get(r, 3) for r in w.rho}
        assert kinds == {0, 1, 2, 3} and len(set(w.want[name])) == MAX


@pytest.mark.parametrize("field", FIELDS)
def test_instances_do_not_depend_on_their_neighbours(ctx, world, field):
    """a later window of the instances, in another order: every result is its own instance's"""
    w = world(field)
    qs = [40, 7, 63, 8, 9, 41, 0]
    same(w.call(ctx, "split", qs), [w.want["split"][q] for q in qs], w.m)


@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("field", FIELDS)
def test_unit_rows_and_the_zero_vector(ctx, world, field, name):
    w = world(field)
    m = w.m
    split, base, _ = MAPS[name]
    rows = [0, w.long_row, w.n - 1, w.empty_row, None]                         # None: eq_x all zero
    exs = [[1 if r == x else 0 for x in range(w.n)] for r in rows]
    qs = [3, 2, 7, 11, 6]                                                      # whose eq_y
    rhos = [w.rho[3]] * len(qs)                                                # a random one: all three matrices count
    assert rhos[0] not in (0, 1, m - 1)
    want = E.multi_eval(w.triples, m, exs, [w.ey[name][q] for q in qs], rhos, split, base)
    assert want[3] == 0 and want[4] == 0 and all(want[:3])
    got = w.call(ctx, name, qs, dex=[dev(mont(x, m)) for x in exs], rho=rhos)
    same(got, want, m)
    assert not got[3:].any()


@pytest.mark.parametrize("field", FIELDS)
def test_no_stale_partials_from_a_larger_call(ctx, world, field):
    w = world(field)
    same(w.call(ctx, "identity", list(range(MAX))), w.want["identity"], w.m)
    same(w.call(ctx, "identity", [5]), [w.want["identity"][5]], w.m)
    same(w.call(ctx, "split", [6]), [w.want["split"][6]], w.m)


@pytest.mark.parametrize("field", FIELDS)
def test_equals_the_devices_older_sequence(ctx, world, field):
    """eq tables of a random point through vdf_pair_table, then M(r_y) the way the single verifier makes it: vdf_spmv3_t and a dot."""
    w = world(field)
    m = w.m
    rng = np.random.default_rng([59, field])
    k = 10                                                                     # 2^10 = 1024 >= 769 rows and >= 701 columns
    rx, ry, (rho,) = S.rand_ints(rng, m, k), S.rand_ints(rng, m, k), S.rand_ints(rng, m, 1)
    tabs = []
    for r in (rx, ry):
        t = dev(np.full((1 << k, 4), ONES, dtype="<u8"))
        ctx.pair_table(field, mont([(1 - v) % m for v in r], m), mont(r, m), k, t)
        tabs.append(t)
    cols = dev(np.full((w.ncols, 4), ONES, dtype="<u8"))
    ctx.spmv3_t(w.shape, tabs[0], mont([rho], m), cols)
    old = ctx.reduce(field, 0, [cols, tabs[1]], w.ncols)
    ctx.sync()
    ctx.kernel_events()
    out = np.full((1, 4), ONES, dtype="<u8")
    ctx.sparse_eval_multi(w.shape, [tabs[0]], [tabs[1]], mont([rho], m), out=out)
    assert np.array_equal(out, old.reshape(1, 4))
    # ... and both are the spec's value for those tables
    ex, ey = ints(host(tabs[0]).reshape(-1, 4)), ints(host(tabs[1]).reshape(-1, 4))
    ex, ey = [o.from_mont(v, m) for v in ex], [o.from_mont(v, m) for v in ey]
    same(out, E.multi_eval(w.triples, m, [ex], [ey], [rho], w.ncols, 0), m)


def _raw(ctx, w, count, ex, nx, ey, ny, rho, split, base, out):
    arr = lambda ps: None if ps is None else (ctypes.c_void_p * max(len(ps), 1))(*ps)
    return hip.lib.vdf_sparse_eval_multi(ctx.handle, w.shape.handle, count, arr(ex), nx, arr(ey), ny, rho, split, base, out)


@pytest.mark.parametrize("field", FIELDS)
def test_refusals_launch_nothing(ctx, world, field):
    w = world(field)
    m = w.m
    out = np.full((MAX + 1, 4), ONES, dtype="<u8")
    px = [t.data_ptr() for t in w.dex]
    py = [t.data_ptr() for t in w.dey["split"]]
    rho = mont(w.rho + [1], m)
    rp, op = rho.ctypes.data, out.ctypes.data
    n, nc = w.n, w.ncols
    refused = [
        ("count above the cap", (MAX + 1, px + px[:1], n, py + py[:1], 741, rp, 600, 640, op)),
        ("negative count", (-1, px, n, py, 741, rp, 600, 640, op)),
        ("null eq_x", (2, None, n, py[:2], 741, rp, 600, 640, op)),
        ("null eq_y", (2, px[:2], n, None, 741, rp, 600, 640, op)),
        ("null entry of eq_x", (2, [px[0], None], n, py[:2], 741, rp, 600, 640, op)),
        ("null entry of eq_y", (2, px[:2], n, [None, py[1]], 741, rp, 600, 640, op)),
        ("null rho", (2, px[:2], n, py[:2], 741, None, 600, 640, op)),
        ("null out", (2, px[:2], n, py[:2], 741, rp, 600, 640, None)),
        ("nx < num_cons", (2, px[:2], n - 1, py[:2], 741, rp, 600, 640, op)),
        ("col_split > num_cols", (2, px[:2], n, py[:2], 741, rp, nc + 1, 0, op)),
        ("col_split > ny", (2, px[:2], n, py[:2], 599, rp, 600, 0, op)),
        ("the moved columns end past ny", (2, px[:2], n, py[:2], 740, rp, 600, 640, op)),
        ("col_hi_base past ny", (2, px[:2], n, py[:2], 741, rp, nc, 742, op)),
    ]
    for what, args in refused:
        assert _raw(ctx, w, *args) == 1, what                                  # VDF_ERR_BAD_ARG
        assert ctx.kernel_events() == [], what
    assert (out == ONES).all()
    # no instance: VDF_OK, nothing written, nothing launched
    assert _raw(ctx, w, 0, None, 0, None, 0, None, 0, 0, None) == 0
    assert _raw(ctx, w, 0, px, n, py, 741, rp, 600, 640, op) == 0
    assert ctx.kernel_events() == [] and (out == ONES).all()
    with pytest.raises(VdfError) as e:
        ctx.sparse_eval_multi(w.shape, w.dex[:2], w.dey["split"][:2], rho[:2], MAPS["split"][0], 700)
    assert e.value.code == 1
    # the context goes on working, and the exact bound of the map is accepted: ny = 741 = 640 + (701 - 600)
    same(w.call(ctx, "split", [0, 1]), w.want["split"][:2], m)
