"""GPU: the operand block every cross-term entry point of libvdf_hip.so shares -- z2, Az1, Bz1, Cz1, u1, Az2, Bz2, Cz2, T -- checked
the same way at each of the seven: vdf_nifs_cross_term, _rows, _minroot, _minroot_forward, _minroot_forward_lanes, _periodic and
_minroot_fold.

a. Refusals.  Per entry point: each of the eight vectors NULL, each of them in host memory, u1 NULL, u1 in device memory (and r of
   the fold in device memory).  Every case asserts the status code and the text of vdf_last_error, nothing is launched and no
   output is written.  The expected codes and texts below are literals: they are what the library answered before the entry points
   shared one validator, and the entry points differ on purpose (vdf_nifs_cross_term and _rows report a NULL vector as one that
   is not in device memory and a NULL u1 as one that is not in host memory; the periodic call names its description in the text).
   The periodic call's description is host memory too: the struct itself and each array it points to, in device memory, are
   refused with the same code and text, and the struct is not read through before that is known.
b. One good call per entry point at the smallest legal sizes (the built-in circuit's shape at t = 4, the stencils at t = 2, two
   lanes, a description of two rows), exact against big integers over the rows' triples (periodic_spec.sparse_reference).  The
   inputs are distinct random vectors and all four outputs are checked, so an operand wired to the wrong place shows: a swap of
   Az1 and Bz1 alone is invisible in the formula of T, not in its value.  Outputs start as garbage; rows outside the call's range
   must keep it."""
import numpy as np
import pytest

from oracle import pasta as o
from periodic_spec import sparse_reference
from util import dev, host, ints, limbs, mont, rand_limbs
from vdf_amd import hip
from vdf_amd.hip import VdfError

pytestmark = pytest.mark.gpu
FIELD, M = o.FIELD_FQ, o.Q
T_SHAPE, T_STENCIL, LANES = 4, 2, 2
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
VECTORS = ("z2", "az1", "bz1", "cz1", "az2", "bz2", "cz2", "T")
ENTRY_POINTS = ("cross_term", "rows", "minroot", "forward", "forward_lanes", "periodic", "fold")

BAD_ARG = 1                                                           # VDF_ERR_BAD_ARG
NULL = "null argument"
ON_HOST = "scalar operands of fused calls live in host memory"
ON_DEVICE = "vector operands of fused calls live in device memory"
DESCRIPTION = "the description and scalar operands of fused calls live in host memory"
# entry point -> (a vector NULL, a vector in host memory, u1 NULL, u1 in device memory)
SHAPE_CALLS = ((BAD_ARG, ON_DEVICE), (BAD_ARG, ON_DEVICE), (BAD_ARG, ON_HOST), (BAD_ARG, ON_HOST))
STENCIL_CALLS = ((BAD_ARG, NULL), (BAD_ARG, ON_DEVICE), (BAD_ARG, NULL), (BAD_ARG, ON_HOST))
EXPECTED = {"cross_term": SHAPE_CALLS, "rows": SHAPE_CALLS, "minroot": STENCIL_CALLS, "forward": STENCIL_CALLS,
            "forward_lanes": STENCIL_CALLS, "fold": STENCIL_CALLS,
            "periodic": ((BAD_ARG, NULL), (BAD_ARG, ON_DEVICE), (BAD_ARG, NULL), (BAD_ARG, DESCRIPTION))}
R_ON_DEVICE = (BAD_ARG, ON_HOST)                                      # the fold's challenge


def triples(entries):
    """[(row, col, int)] -> (rows, cols, Montgomery values) as Context.shape_create and sparse_reference take them"""
    return (np.array([e[0] for e in entries], dtype=np.uint32), np.array([e[1] for e in entries], dtype=np.uint32),
            mont([e[2] % M for e in entries], M))


def inverse_stencil(t, one_col, row0):
    """Rows 0 .. 3t of the built-in circuit at t (oracle.pasta.step_circuit_shape: z_in at 0 .. 2, the rounds from 3 on), moved to
    row0, with the constant's column moved to one_col"""
    sh = o.step_circuit_shape(t, FIELD)
    move = lambda es: [(r + row0, one_col if c == sh.num_vars else c, v) for r, c, v in es if r <= 3 * t]
    assert all(c < 3 + 4 * t + 1 or c == sh.num_vars for es in (sh.A, sh.B, sh.C) for r, c, v in es if r <= 3 * t)
    return [triples(move(es)) for es in (sh.A, sh.B, sh.C)]


def forward_stencil(t, lanes, seg_begin, one_col, row0):
    """The rows include/vdf_hip.h states for vdf_nifs_cross_term_minroot_forward_lanes"""
    A, B, C = [], [], []
    for l in range(lanes):
        S, Z, R = seg_begin + l * (3 * t + 1), seg_begin - 3 * lanes + 3 * l, row0 + l * (3 * t + 1)
        for j in range(t):
            x, t1, t2 = S + 3 * j, S + 3 * j + 1, S + 3 * j + 2
            A += [(R + 3 * j, x, 1), (R + 3 * j + 1, t1, 1), (R + 3 * j + 2, t2, 1)]
            B += [(R + 3 * j, x, 1), (R + 3 * j + 1, t1, 1), (R + 3 * j + 2, x, 1)]
            C += [(R + 3 * j, t1, 1), (R + 3 * j + 1, t2, 1)]
            if j == 0:
                C += [(R + 2, Z, 1), (R + 2, Z + 1, 1)]
            else:
                C += [(R + 3 * j + 2, S + 3 * (j - 1), 1), (R + 3 * j + 2, S + 3 * (j - 2) if j >= 2 else Z, 1),
                      (R + 3 * j + 2, Z + 2, 1), (R + 3 * j + 2, one_col, j - 1)]
        A.append((R + 3 * t, S + 3 * t, 1))
        B.append((R + 3 * t, one_col, 1))
        C += [(R + 3 * t, Z + 2, 1), (R + 3 * t, one_col, t)]
    return [triples(es) for es in (A, B, C)]


# a description of two rows over two variables (v0, v1) per repetition j, with every way a coefficient is applied:
#   row 0:  v0 * (5 v1) = (7 + 3 (j - j0)) one - v0          row 1:  z[1] * v0 = 5 v1 + (2 + (j - j0)) one
P_CONSTS = (1, 5, 7, 3, M - 1, 2)
P_SEG_BEGIN, P_J0, P_REPS, P_ROW0 = 3, 0, 2, 1


def periodic_description(one_col):
    pr = hip.PeriodicRows()
    terms = [[(hip.TERM_SEG, 0, 0, 0xFF)], [(hip.TERM_SEG, 1, 1, 0xFF)], [(hip.TERM_ABS, one_col, 2, 3), (hip.TERM_SEG, 0, 4, 0xFF)],
             [(hip.TERM_ABS, 1, 0, 0xFF)], [(hip.TERM_SEG, 0, 0, 0xFF)], [(hip.TERM_SEG, 1, 1, 0xFF), (hip.TERM_ABS, one_col, 5, 0)]]
    n = 0
    for q, lst in enumerate(terms):
        for kind, col, c0, c1 in lst:
            pr.terms[n].kind, pr.terms[n].col, pr.terms[n].c0, pr.terms[n].c1 = kind, col, c0, c1
            n += 1
        pr.row_start[q + 1] = n
    pr.consts[:len(P_CONSTS)] = mont(P_CONSTS, M)
    pr.c.n_cons, pr.c.n_vars, pr.c.j0, pr.c.n_terms, pr.c.n_consts = 2, 2, P_J0, n, len(P_CONSTS)
    return pr


def periodic_triples(one_col):
    A, B, C = [], [], []
    for j in range(P_J0, P_J0 + P_REPS):
        v0, v1, r = P_SEG_BEGIN + 2 * j, P_SEG_BEGIN + 2 * j + 1, P_ROW0 + 2 * (j - P_J0)
        A += [(r, v0, 1), (r + 1, 1, 1)]
        B += [(r, v1, 5), (r + 1, v0, 1)]
        C += [(r, one_col, 7 + 3 * (j - P_J0)), (r, v0, M - 1), (r + 1, v1, 5), (r + 1, one_col, 2 + (j - P_J0))]
    return [triples(es) for es in (A, B, C)]


class World:
    """The shape, the operands (never changed) and, per entry point, its call and the rows and triples of its reference"""

    def __init__(self, ctx):
        sh = o.step_circuit_shape(T_SHAPE, FIELD)
        self.nc, self.ncols, self.one = sh.num_cons, sh.num_vars + 1 + sh.num_io, sh.num_vars
        self.mats = [triples(es) for es in (sh.A, sh.B, sh.C)]
        self.shape = ctx.shape_create(FIELD, self.nc, self.ncols, self.mats)
        rng = np.random.default_rng(23)
        self.z2, self.u1, self.r = rand_limbs(rng, self.ncols), rand_limbs(rng, 1), rand_limbs(rng, 1)
        self.abc1 = [rand_limbs(rng, self.nc) for _ in range(3)]
        self.prev = [rand_limbs(rng, self.nc) for _ in range(5)]       # the fold: A z2, B z2, C z2, T of the step before, and E1
        assert len({x.tobytes() for x in self.abc1 + self.prev}) == 8
        self.pr = periodic_description(self.one)
        t, nr, one = T_STENCIL, 3 * T_STENCIL + 1, self.one
        assert self.one >= 6 + LANES * nr and 3 + LANES * nr <= self.nc
        # name -> (call(ops), row_begin, row_count, triples of those rows)
        c = ctx
        self.entry = {
            "cross_term": (lambda p: c.nifs_cross_term(self.shape, *p), 0, self.nc, self.mats),
            "rows": (lambda p: c.nifs_cross_term_rows(self.shape, 3, 5, 1, *p), 3, 5, self.mats),
            "minroot": (lambda p: c.nifs_cross_term_minroot(FIELD, 4, t, 3, one, 2, *p), 2, nr, inverse_stencil(t, one, 2)),
            "forward": (lambda p: c.nifs_cross_term_minroot_forward(FIELD, t, 3, one, 1, *p), 1, nr, forward_stencil(t, 1, 3, one, 1)),
            "forward_lanes": (lambda p: c.nifs_cross_term_minroot_forward_lanes(FIELD, t, LANES, 3 * LANES, one, 3, *p), 3, LANES * nr,
                              forward_stencil(t, LANES, 3 * LANES, one, 3)),
            "periodic": (lambda p: c.nifs_cross_term_periodic(FIELD, self.pr, P_J0, P_REPS, P_SEG_BEGIN, P_ROW0, self.ncols, self.nc, *p),
                         P_ROW0, 2 * P_REPS, periodic_triples(one)),
            "fold": (lambda p: c.nifs_cross_term_minroot_fold(FIELD, 4, t, 3, one, 5, p[0], p[9], *p[1:4], p[10], p[11], *p[4:9]), 5, nr,
                     inverse_stencil(t, one, 5)),
        }

    def operands(self, name):
        """Fresh device buffers in the wrappers' order z2, az1, bz1, cz1, u1, az2, bz2, cz2, T (the fold: then r, E1, T_prev = T).
        The outputs are garbage, but for the fold, whose outputs are the previous step's vectors on the way in."""
        fold = name == "fold"
        outs = [dev(x) for x in self.prev[:4]] if fold else [dev(np.full((self.nc, 4), ONES - np.uint64(k), dtype="<u8")) for k in range(4)]
        p = [dev(self.z2)] + [dev(x) for x in self.abc1] + [self.u1] + outs
        return p + [self.r, dev(self.prev[4]), outs[3]] if fold else p


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.shape.free()


@pytest.fixture(autouse=True)
def timed(ctx):
    ctx.set_kernel_timing(True)
    ctx.kernel_events()
    yield
    ctx.kernel_events()
    ctx.set_kernel_timing(False)


def fold_rows(x, r, y, rb, n):
    """x[rb:rb + n] + r * y[rb:rb + n] over big integers, the other rows of x as they are (Montgomery limbs in and out)"""
    fm = lambda a: [o.from_mont(v, M) for v in ints(a)]
    out = x.copy()
    (rr,) = fm(r)
    out[rb:rb + n] = mont([(a + rr * b) % M for a, b in zip(fm(x[rb:rb + n]), fm(y[rb:rb + n]))], M)
    return out


# ---- b. one good call per entry point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_a_good_call_reads_and_writes_every_operand_in_its_place(ctx, world, name):
    w = world
    call, rb, n, mats = w.entry[name]
    p = w.operands(name)
    before = [host(x).copy() for x in p[5:9]]
    call(p)
    ctx.sync()
    abc1 = w.abc1
    if name == "fold":                                                  # the running rows folded with the previous fresh ones first
        abc1 = [fold_rows(x, w.r, y, rb, n) for x, y in zip(w.abc1, w.prev[:3])]
        for k in range(3):
            assert np.array_equal(host(p[1 + k]), abc1[k]), ("running vector", k)
        assert np.array_equal(host(p[10]), fold_rows(w.prev[4], w.r, w.prev[3], rb, n)), "E1"
    else:
        for k in range(3):
            assert np.array_equal(host(p[1 + k]), w.abc1[k]), ("an input was written", k)
    assert np.array_equal(host(p[0]), w.z2)
    want = sparse_reference(FIELD, mats, rb, n, w.z2, *abc1, w.u1)
    for what, got, e, b in zip(("Az2", "Bz2", "Cz2", "T"), p[5:9], want, before):
        g = host(got)
        assert np.array_equal(g[rb:rb + n], e), (name, what)
        assert np.array_equal(g[:rb], b[:rb]) and np.array_equal(g[rb + n:], b[rb + n:]), (name, what, "written outside the rows")


# ---- a. refusals ----------------------------------------------------------------------------------------------------------------
def refused(ctx, world, name, p, want, what):
    call = world.entry[name][0]
    kept = [(x, host(x).copy()) for x in p[:12] if hasattr(x, "data_ptr")]
    with pytest.raises(VdfError) as e:
        call(p)
    assert (e.value.code, str(e.value)) == (want[0], f"vdf_hip error {want[0]}: {want[1]}"), (name, what)
    assert ctx.kernel_events() == [], (name, what)
    ctx.sync()
    for x, b in kept:
        assert np.array_equal(host(x), b), (name, what, "a vector changed")


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_every_misplaced_operand_is_refused_with_the_same_code_and_text_as_ever(ctx, world, name):
    null_vec, host_vec, null_u1, dev_u1 = EXPECTED[name]
    at = {v: (0, 1, 2, 3, 5, 6, 7, 8)[k] for k, v in enumerate(VECTORS)}
    for v in VECTORS:
        p = world.operands(name)
        p[at[v]] = None
        refused(ctx, world, name, p, null_vec, v + " NULL")
        p = world.operands(name)
        p[at[v]] = host(p[at[v]]).copy()
        refused(ctx, world, name, p, host_vec, v + " in host memory")
    p = world.operands(name)
    p[4] = None
    refused(ctx, world, name, p, null_u1, "u1 NULL")
    p = world.operands(name)
    p[4] = dev(world.u1)
    refused(ctx, world, name, p, dev_u1, "u1 in device memory")
    if name == "fold":
        p = world.operands(name)
        p[9] = dev(world.r)
        refused(ctx, world, name, p, R_ON_DEVICE, "r in device memory")


def test_a_periodic_description_in_device_memory_is_refused(ctx, world):
    """The struct in device memory holds the host arrays' addresses: a library that read through it would find nothing else wrong."""
    import ctypes
    w, pr = world, world.pr
    want = (BAD_ARG, DESCRIPTION)

    def call_with(description):
        return lambda p: ctx._check(hip.lib.vdf_nifs_cross_term_periodic(ctx.handle, FIELD, description, P_J0, P_REPS, P_SEG_BEGIN, P_ROW0, w.ncols,
                                                                         w.nc, *[hip._ptr(x) for x in p]))

    def dev_bytes(b):
        a = np.zeros((len(b) + 7) // 8 * 8, dtype=np.uint8)
        a[:len(b)] = np.frombuffer(b, dtype=np.uint8)
        return dev(a)
    d_struct = dev_bytes(bytes(pr.c))
    on_device = {"row_start": dev_bytes(pr.row_start.tobytes()), "terms": dev_bytes(bytes(pr.terms)), "consts": dev(pr.consts)}
    keep = w.entry["periodic"]
    try:
        w.entry["periodic"] = (call_with(d_struct.data_ptr()), *keep[1:])
        refused(ctx, w, "periodic", w.operands("periodic"), want, "the description struct in device memory")
        for member, d in on_device.items():
            c = type(pr.c).from_buffer_copy(bytes(pr.c))
            setattr(c, member, ctypes.cast(d.data_ptr(), type(getattr(c, member))) if member == "terms" else d.data_ptr())
            w.entry["periodic"] = (call_with(ctypes.addressof(c)), *keep[1:])
            refused(ctx, w, "periodic", w.operands("periodic"), want, member + " in device memory")
    finally:
        w.entry["periodic"] = keep
    call, rb, n, mats = keep                                            # and the description still works
    p = w.operands("periodic")
    call(p)
    ctx.sync()
    assert np.array_equal(host(p[8])[rb:rb + n], sparse_reference(FIELD, mats, rb, n, w.z2, *w.abc1, w.u1)[3])
