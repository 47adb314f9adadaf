"""GPU: every switchable path of the bucket-method MSM (vdf_amd/csrc/msm.hip) at sizes where the path does real work,
checked exactly against the big-integer oracle (oracle/pasta.py): the surplus beyond MAX_GIANTS shared buckets, the
GIANT_PARTS cap, each vdf_hip_tuning kernel switch, the fine_max = 8 sort geometry, a context's own accumulate fill,
equal / opposite / identity slice heads in the fix-up, batches and jobs, and the signed-digit edges of every window.

A host model of the plan (plan_model, CPU only) predicts from the scalars which path a case reaches; the cases assert
that prediction before they run, so a change of msm.hip's constants shows up as a failing precondition rather than as a
test that quietly covers less.  The model's own checks carry no gpu mark."""
import contextlib
import ctypes

import numpy as np
import pytest

from oracle import pasta as o
from util import limbs, ints, jac_to_affine, rand_limbs

CURVES = [o.CURVE_PALLAS, o.CURVE_VESTA]

# ---- mirrored from vdf_amd/csrc/msm.hip (keep in step: a change there must change these) ----------------------------------
HEAVY_MIN = 6            # HEAVY_MIN
GIANT_SPAN = 64          # GIANT_SPAN
GIANT_CHUNK = 32         # GIANT_CHUNK
GIANT_PARTS = 256        # GIANT_PARTS
MAX_GIANTS = 192         # MAX_GIANTS
ACC_WG_PER_CU = 3        # ACC_WG_PER_CU: the automatic fill of a single MSM of >= 2^22 (scalar, window) entries
ACC_WG_FILL = 2          # ACC_WG_FILL: below that, and in batches
MIN_SLICE = 8            # slice_len(): at least 8 entries per k_accumulate slice
CAP_SPAN = GIANT_PARTS * GIANT_CHUNK       # a giant spanning more slices than this hits the GIANT_PARTS cap
SORT_MAX_BINS = 8192     # msm_make_plan: pass A keeps a cursor per partition in LDS
CU_DEFAULT = 256         # MI355X; the GPU tests read the device's own count

N_BIG = 1 << 18          # the matrix's generator set (Pallas)
SEED_BIG = 0x9A75
C_BIG = 16
N_CAP = 8 * (256 * 127 + 64)          # 260608: a bucket of N_CAP entries at slices of 8 spans 32575 = 127 * 256 + 63 slices
BATCH = [("few64", 200000, 3), ("uniform", 30000, 190000), ("all_equal", 40000, 222000), ("uniform", 129, N_BIG - 129)]  # (dist, n, offset)

# equal slice heads: 2^16 copies of one point under one scalar, and the fix-up route each tuning forces
N_EQ = 1 << 16
EQ_SCALAR = 0x2F0C_5B3A_91D7_E466_0183_22AB_7C5D_F9E1_44B0_6A2D_3C8E_9F17_5D02_B8C4_E6F1_A3   # < 2^246
ROUTES = {"direct": dict(heavy_min=4096, giant_span=1 << 20), "heavy": dict(heavy_min=1, giant_span=1 << 20), "giant": {}}
# (slice_len, route); not (8, "direct"): 2^16 entries at slices of 8 span 8191 slices, beyond the largest heavy_min (4096)
EQ_ROUTES = [(8, "heavy"), (8, "giant"), (64, "direct"), (64, "heavy"), (64, "giant")]


# ---- host model of the plan ------------------------------------------------------------------------------------------------
def signed_digits(sc, c):
    """uint64[n, 4] scalars -> (signed digits int64[n, windows], count of zero-magnitude digits with the sign set), mirroring
    msm.hip DigitIter::next: raw = window + carry; raw > 2^(c-1) gives magnitude 2^c - raw, the sign, and a carry."""
    s = np.ascontiguousarray(sc, dtype="<u8").reshape(-1, 4)
    n = s.shape[0]
    windows = (256 + c - 1) // c
    ext = np.zeros((n, 5), dtype=np.uint64)
    ext[:, :4] = s
    mask, half = np.uint64((1 << c) - 1), 1 << (c - 1)
    carry = np.zeros(n, dtype=np.int64)
    digits = np.zeros((n, windows), dtype=np.int64)
    zero_signed = 0
    for w in range(windows):
        bit = w * c
        limb, sh = bit >> 6, bit & 63
        v = ext[:, limb] >> np.uint64(sh)
        if sh:
            v = v | (ext[:, limb + 1] << np.uint64(64 - sh))
        raw = (v & mask).astype(np.int64) + carry
        over = raw > half
        zero_signed += int(np.count_nonzero(raw == (1 << c)))
        digits[:, w] = np.where(over, raw - (1 << c), raw)
        carry = over.astype(np.int64)
    return digits, zero_signed


def sort_geometry(gsets, c, num_cus, part_bits=-1, sort_staged=1):
    """(pb, fb): partition bits of pass A and fine bits of pass B, as msm_make_plan chooses them."""
    pb = 0
    while pb < c - 1 and (gsets << pb) < num_cus:
        pb += 1
    if 0 <= part_bits <= c - 1:
        pb = part_bits
    fine_max = 8 if c >= 18 and part_bits < 0 and not sort_staged else 10
    while c - 1 - pb > fine_max:
        pb += 1
    while pb > 0 and (gsets << pb) > SORT_MAX_BINS:
        pb -= 1
    return pb, c - 1 - pb


def plan_model(groups, c, num_cus, sets=0, slice_len=0, fill=0, heavy_min=0, giant_span=0):
    """Bucket sizes and fix-up routes of one call over `groups` (a list of uint64[n, 4] scalar vectors), as msm_make_plan,
    k_fine, slice_len and k_fixup see them.  sets = 0: a table-less call (one bucket set per window); sets >= 1: a fixed-base
    table of that many sets.  Entries are sorted by key = (group * sets + window % sets) * 2^(c-1) + magnitude - 1."""
    windows = (256 + c - 1) // c
    if sets <= 0:
        sets = windows
    nbk = 1 << (c - 1)
    gsets = len(groups) * sets
    nkeys = gsets * nbk
    counts = np.zeros(nkeys, dtype=np.int64)
    top_hits = zero_signed = 0
    for g, sc in enumerate(groups):
        d, z = signed_digits(sc, c)
        zero_signed += z
        mag = np.abs(d)
        top_hits += int(np.count_nonzero(mag == nbk))
        w = np.broadcast_to(np.arange(windows), mag.shape)
        live = mag > 0
        keys = (g * sets + w[live] % sets) * nbk + mag[live] - 1
        counts += np.bincount(keys, minlength=nkeys)
    n_all = sum(int(np.asarray(sc).reshape(-1, 4).shape[0]) for sc in groups)
    if fill == 0:
        fill = ACC_WG_PER_CU if len(groups) == 1 and n_all * windows >= 1 << 22 else ACC_WG_FILL
    slots = num_cus * fill * 256
    ne = int(counts.sum())
    L = slice_len if slice_len else max(MIN_SLICE, -(-ne // slots))
    ends = np.cumsum(counts)
    starts = ends - counts
    live = counts > 0
    tf, tl = starts[live] // L, (ends[live] - 1) // L
    span = tl - tf
    heavy_span = max(2 * ((ne // nkeys + L - 1) // L) + 4, heavy_min or HEAVY_MIN)
    heavy = span > heavy_span
    giant = heavy & (span > (giant_span or GIANT_SPAN))
    gspan = span[giant]
    parts = np.minimum(GIANT_PARTS, -(-gspan // GIANT_CHUNK))
    chunk = -(-gspan // np.maximum(parts, 1))
    empty_parts = parts - (-(-gspan // np.maximum(chunk, 1)))          # trailing parts whose chunk starts past the last head
    return dict(L=L, slots=slots, ne=ne, counts=counts, span_max=int(span.max()) if span.size else 0,
                heads=int(span.sum()), plain_heavy=int(np.count_nonzero(heavy & ~giant)), giants=int(np.count_nonzero(giant)),
                capped=int(np.count_nonzero(gspan > CAP_SPAN)), empty_parts=int(empty_parts.max()) if gspan.size else 0,
                top_hits=top_hits, zero_signed=zero_signed)


# ---- scalar distributions aimed at paths -----------------------------------------------------------------------------------
def edge_value(c, digit):
    """Every window below bit 253 holds the raw digit `digit` (so the value stays below both scalar moduli)."""
    return sum(digit << (w * c) for w in range(253 // c))


def ones_carry_values(c, k, rng):
    """k values in which a window that carries (raw digit 2^(c-1) + 1) is followed by 1..3 windows of all ones: with the carry
    those windows read exactly 2^c, the zero-magnitude signed digit that pass A must skip while passing the carry on."""
    half, mask, top = 1 << (c - 1), (1 << c) - 1, 250 // c
    vals = []
    for _ in range(k):
        run = int(rng.integers(1, 4))
        w0 = int(rng.integers(0, max(1, top - run - 1)))
        low = int(rng.integers(0, 1 << 62)) % (1 << (w0 * c)) if w0 else 0
        v = low + ((half + 1) << (w0 * c)) + sum(mask << ((w0 + j) * c) for j in range(1, run + 1))
        assert v.bit_length() <= 250
        vals.append(v)
    return vals


def make_scalars(dist, n, c, seed):
    """uint64[n, 4] scalars of one named distribution for window c; every value is below both scalar moduli."""
    rng = np.random.default_rng(seed)
    if dist == "uniform":
        return rand_limbs(rng, n)
    if dist.startswith("few"):                                           # few1, few2, few64: drawn from k random values
        k = int(dist[3:])
        return rand_limbs(rng, k)[rng.integers(0, k, size=n)].copy()
    if dist == "all_equal":
        return np.repeat(rand_limbs(rng, 1), n, axis=0).copy()
    sc = rand_limbs(rng, n)                                              # the edge cases: mixed into random scalars
    half = 1 << (c - 1)
    if dist == "top_digit":
        sc[0::2] = limbs([edge_value(c, half)])[0]
    elif dist == "top_digit1":
        sc[0::2] = limbs([edge_value(c, half + 1)])[0]
    elif dist == "ones_carry":
        pool = limbs(ones_carry_values(c, 64, rng))
        sc[0::2] = pool[rng.integers(0, 64, size=(n + 1) // 2)]
    else:
        raise KeyError(dist)
    return sc


# ---- CPU: the model itself and the preconditions it promises ----------------------------------------------------------------
@pytest.mark.parametrize("c", [4, 7, 11, 13, 16, 17, 19, 20])
def test_model_digits_recompose_the_scalar(c):
    rng = np.random.default_rng(c)
    sc = np.concatenate([rand_limbs(rng, 64), limbs([edge_value(c, 1 << (c - 1)), edge_value(c, (1 << (c - 1)) + 1)]),
                         limbs(ones_carry_values(c, 32, rng)), limbs([0, 1, (1 << 254) - 1, o.P - 1, o.Q - 1])])
    d, _ = signed_digits(sc, c)
    assert np.abs(d).max() <= 1 << (c - 1)
    for v, row in zip(ints(sc), d):
        assert sum(int(x) << (w * c) for w, x in enumerate(row)) == v


@pytest.mark.parametrize("c", [4, 7, 11, 13, 16, 17, 19, 20])
def test_model_edge_distributions_reach_their_digits(c):
    """top_digit puts every window below bit 253 into the top bucket 2^(c-1); ones_carry yields zero-magnitude signed digits."""
    n = 3000
    per = 253 // c
    assert plan_model([make_scalars("top_digit", n, c, 5)], c, CU_DEFAULT)["top_hits"] >= (n // 2) * per
    d, _ = signed_digits(make_scalars("top_digit1", n, c, 5)[0:1], c)      # 2^(c-1) + 1 in every window: a chain of carries
    half = 1 << (c - 1)
    assert d[0, 0] == -(half - 1) and (d[0, 1:per] == -(half - 2)).all() and d[0, per] == 1
    assert plan_model([make_scalars("ones_carry", n, c, 5)], c, CU_DEFAULT)["zero_signed"] >= n // 2


def test_model_few_distinct_exceeds_max_giants():
    """few_distinct(64) at 2^18, window 16, no endomorphism, 256 CUs: ~1000 buckets of ~4000 entries, each a giant."""
    sc = make_scalars("few64", N_BIG, C_BIG, 1)
    for sets in (0, 1, 2):
        m = plan_model([sc], C_BIG, CU_DEFAULT, sets=sets)
        assert m["giants"] >= 2 * MAX_GIANTS, (sets, m["giants"])


def test_model_all_equal_passes_the_parts_cap_with_empty_trailing_parts():
    m = plan_model([make_scalars("all_equal", N_CAP, C_BIG, 2)], C_BIG, CU_DEFAULT, slice_len=8)
    assert m["capped"] >= 8 and m["span_max"] > 3 * CAP_SPAN and m["empty_parts"] >= 1


def test_model_batch_exceeds_max_giants():
    for sets in (0, 1):
        m = plan_model(batch_groups(), C_BIG, CU_DEFAULT, sets=sets)
        assert m["giants"] >= 2 * MAX_GIANTS, (sets, m["giants"])


@pytest.mark.parametrize("c", [18, 19, 20])
def test_model_fine_max_changes_the_sort(c):
    """sort_staged = 0 at windows >= 18 caps pass B at 2^8 fine buckets (msm_make_plan fine_max): over a one-set table the
    partitions take the surplus bits; table-less at 20 bits the 8192-partition limit wins and the geometry is unchanged."""
    staged, unstaged = sort_geometry(1, c, CU_DEFAULT, sort_staged=1), sort_geometry(1, c, CU_DEFAULT, sort_staged=0)
    assert unstaged[1] == 8 and staged != unstaged
    assert sort_geometry(1, c, CU_DEFAULT, part_bits=12, sort_staged=0)[0] == 12      # a fixed part_bits turns it off


@pytest.mark.parametrize("slen,route", EQ_ROUTES)
def test_model_equal_head_routes(slen, route):
    assert_route(equal_points_model(slen, route, CU_DEFAULT), route)


# ---- GPU helpers -------------------------------------------------------------------------------------------------------------
def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def tuned(**fields):
    from vdf_amd import hip
    base = hip.tuning_get()
    try:
        if fields:
            hip.tuning_set(**fields)
        yield
    finally:
        hip.lib.vdf_hip_tuning_set(ctypes.byref(base))


@contextlib.contextmanager
def window(ctx, c):
    ctx.set_msm_window(c)
    try:
        yield
    finally:
        ctx.set_msm_window(0)


def aff(jac, curve):
    return jac_to_affine(jac, curve)


class BigSet:
    """The matrix's generators: 2^18 synthetic Pallas points, a copy with a (16, 1) table and one with a (16, 2) table;
    scalars and their references cached by distribution."""

    def __init__(self, ctx):
        self.curve = o.CURVE_PALLAS
        self.plain = ctx.bases_generate(self.curve, SEED_BIG, N_BIG)
        self.tbl1 = ctx.bases_generate(self.curve, SEED_BIG, N_BIG)
        self.tbl1.precompute(C_BIG, 1)
        self.tbl2 = ctx.bases_generate(self.curve, SEED_BIG, N_BIG)
        self.tbl2.precompute(C_BIG, 2)
        self.cache = {}
        self.checked = set()

    def case(self, dist):
        if dist not in self.cache:
            sc = make_scalars(dist, N_BIG, C_BIG, 1)
            self.cache[dist] = (sc, o.msm_by_dlog_limbs(sc, self.curve, SEED_BIG))
        return self.cache[dist]

    def free(self):
        for b in (self.plain, self.tbl1, self.tbl2):
            b.free()


@pytest.fixture(scope="module")
def big(ctx):
    s = BigSet(ctx)
    yield s
    s.free()


MODES = ["w16", "glv", "tbl16x1", "tbl16x2"]


def run_mode(ctx, big, mode, sc):
    """w16: table-less at window 16 (a fixed window never takes the endomorphism); glv: table-less, automatic window, the whole
    set (the endomorphism unless glv = 0); tblCxS: over a fixed-base table."""
    if mode == "w16":
        with window(ctx, C_BIG):
            return aff(ctx.msm(big.plain, sc), big.curve)
    if mode == "glv":
        return aff(ctx.msm(big.plain, sc), big.curve)
    return aff(ctx.msm(big.tbl1 if mode == "tbl16x1" else big.tbl2, sc), big.curve)


def mode_sets(mode):
    return {"w16": 0, "tbl16x1": 1, "tbl16x2": 2}[mode]


# ---- 2: the tuning matrix ----------------------------------------------------------------------------------------------------
VARIANTS = {
    "default": {}, "fixup_quad": dict(fixup_serial=0), "fine_unstaged": dict(sort_staged=0), "segments": dict(reduction=0),
    "segments_q64": dict(reduction=0, reduction_quads=64), "segments_q65536": dict(reduction=0, reduction_quads=65536),
    "part_bits0": dict(part_bits=0), "part_bits_top": dict(part_bits=C_BIG - 1), "slice1": dict(slice_len=1),
    "slice8": dict(slice_len=8), "slice4096": dict(slice_len=4096), "heavy1_giant16": dict(heavy_min=1, giant_span=16),
    "heavy4096_nogiant": dict(heavy_min=4096, giant_span=1 << 20), "quad_heavy2_giant16": dict(fixup_serial=0, heavy_min=2, giant_span=16),
    "fill1": dict(accumulate_fill=1), "fill3": dict(accumulate_fill=3), "lds55296": dict(accumulate_lds=55296), "glv0": dict(glv=0)}
MATRIX = [(v, d, m) for v in VARIANTS for d in ("few64", "all_equal", "uniform") for m in MODES]
MATRIX += [(v, d, m) for v in ("default", "fixup_quad", "segments", "slice8")
           for d in ("few1", "few2", "top_digit", "top_digit1", "ones_carry") for m in MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,dist,mode", MATRIX, ids=["-".join(x) for x in MATRIX])
def test_tuning_matrix(ctx, big, variant, dist, mode):
    sc, want = big.case(dist)
    if mode != "glv" and (dist, mode) not in big.checked and dist in ("few64", "all_equal"):
        # the path each hot case is here for, with this device's CU count and the default tuning
        m = plan_model([sc], C_BIG, num_cus(), sets=mode_sets(mode))
        assert m["giants"] >= (2 * MAX_GIANTS if dist == "few64" else 1), m["giants"]
        if dist == "all_equal":
            assert m["capped"] >= 1
        big.checked.add((dist, mode))
    with tuned(**VARIANTS[variant]):
        got = run_mode(ctx, big, mode, sc)
    assert got == want, (variant, dist, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("serial", [1, 0], ids=["serial", "quad"])
@pytest.mark.parametrize("mode", ["w16", "tbl16x1"])
def test_giant_parts_cap_with_empty_trailing_parts(ctx, big, mode, serial):
    """All-equal scalars with slices of 8: every giant spans ~32 600 slices, past the GIANT_PARTS cap, and the cap's chunking
    leaves its last part empty (it stores the identity and still arrives)."""
    sc = make_scalars("all_equal", N_CAP, C_BIG, 2)
    m = plan_model([sc], C_BIG, num_cus(), sets=mode_sets(mode), slice_len=8)
    assert m["capped"] >= 1 and m["empty_parts"] >= 1, m
    want = o.msm_by_dlog_limbs(sc, big.curve, SEED_BIG)
    with tuned(slice_len=8, fixup_serial=serial):
        assert run_mode(ctx, big, mode, sc) == want




@pytest.mark.gpu
@pytest.mark.parametrize("c", [18, 19, 20])
def test_fine_max_8_sort_geometry(ctx, c):
    """Windows of 18 bits and more with sort_staged = 0 and part_bits = -1: pass B keeps at most 2^8 fine buckets."""
    curve, n, seed = o.CURVE_PALLAS, 1 << 16, 0xF1AE
    assert sort_geometry(1, c, num_cus(), sort_staged=0) != sort_geometry(1, c, num_cus(), sort_staged=1)
    bases = ctx.bases_generate(curve, seed, n)
    cases = [(d, make_scalars(d, n, c, c)) for d in ("uniform", "few64")]
    want = {d: o.msm_by_dlog_limbs(sc, curve, seed) for d, sc in cases}
    try:
        with tuned(sort_staged=0, part_bits=-1), window(ctx, c):
            for d, sc in cases:
                assert aff(ctx.msm(bases, sc), curve) == want[d], ("table-less", d)
            bases.precompute(c, 1)
            for d, sc in cases:
                assert aff(ctx.msm(bases, sc), curve) == want[d], ("table", d)
    finally:
        bases.free()


@pytest.mark.gpu
def test_per_context_accumulate_fill(ctx, big):
    """vdf_ctx_set_accumulate_fill on a second context (the session context keeps its own): fills 1, 2, 3, then 0."""
    import vdf_amd
    cases = [big.case(d) for d in ("few64", "uniform", "all_equal")]
    with vdf_amd.Context(0) as c2:
        for fill in (1, 2, 3, 0):
            c2.set_accumulate_fill(fill)
            for sc, want in cases:
                with window(c2, C_BIG):
                    assert aff(c2.msm(big.plain, sc), big.curve) == want, (fill, "w16")
                assert aff(c2.msm(big.tbl1, sc), big.curve) == want, (fill, "tbl16x1")
    for sc, want in cases[:1]:
        assert run_mode(ctx, big, "w16", sc) == want


# ---- 3: equal, opposite and identity slice heads -----------------------------------------------------------------------------


def equal_points_model(slen, route, cus):
    sc = limbs([EQ_SCALAR] * N_EQ)
    t = ROUTES[route]
    return plan_model([sc], C_BIG, cus, slice_len=slen, heavy_min=t.get("heavy_min", 0), giant_span=t.get("giant_span", 0))


def assert_route(m, route):
    if route == "direct":
        assert m["plain_heavy"] == 0 and m["giants"] == 0 and m["span_max"] >= 2, m
    elif route == "heavy":
        assert m["plain_heavy"] >= 1 and m["giants"] == 0, m
    else:
        assert m["giants"] >= 1, m




def point_set(curve, n, alternate):
    from util import affine_array
    m = o.curve_base_modulus(curve)
    P = o.pt_mul(0xC0FFEE, o.generator(curve), m)
    arr = np.repeat(affine_array([P], curve), n, axis=0)
    if alternate:
        arr[1::2] = affine_array([o.pt_neg(P, m)], curve)[0]
    return P, m, arr


@pytest.mark.gpu
@pytest.mark.parametrize("serial", [1, 0], ids=["serial", "quad"])
@pytest.mark.parametrize("slen,route", EQ_ROUTES)
@pytest.mark.parametrize("curve", CURVES, ids=["pallas", "vesta"])
def test_equal_slice_heads(ctx, curve, slen, route, serial):
    """2^16 copies of one point with one scalar: every slice head of the 16 hot buckets is the same point, so the fix-up's
    additions (k_fixup / k_fixup_serial, the heavy wave sum, the giants' parts and their combine) meet P + P."""
    assert_route(equal_points_model(slen, route, num_cus()), route)
    P, m, arr = point_set(curve, N_EQ, alternate=False)
    r = o.curve_scalar_modulus(curve)
    bases = ctx.bases_upload(curve, arr)
    try:
        with tuned(slice_len=slen, fixup_serial=serial, **ROUTES[route]), window(ctx, C_BIG):
            got = aff(ctx.msm(bases, limbs([EQ_SCALAR] * N_EQ)), curve)
    finally:
        bases.free()
    assert got == o.pt_mul(N_EQ * EQ_SCALAR % r, P, m)


@pytest.mark.gpu
@pytest.mark.parametrize("serial", [1, 0], ids=["serial", "quad"])
@pytest.mark.parametrize("slen,route", [(8, "giant"), (8, "heavy"), (64, "direct"), (64, "giant")])
def test_opposite_and_identity_slice_heads(ctx, slen, route, serial):
    """P and -P alternating under one scalar: slice heads are small multiples of P, the identity among them, and opposite
    pairs meet in the fix-up.  Odd n leaves s P, even n the identity."""
    curve = o.CURVE_PALLAS
    r = o.curve_scalar_modulus(curve)
    for n in (N_EQ + 1, N_EQ):
        P, m, arr = point_set(curve, n, alternate=True)
        bases = ctx.bases_upload(curve, arr)
        try:
            with tuned(slice_len=slen, fixup_serial=serial, **ROUTES[route]), window(ctx, C_BIG):
                got = aff(ctx.msm(bases, limbs([EQ_SCALAR] * n)), curve)
        finally:
            bases.free()
        assert got == (o.pt_mul(EQ_SCALAR % r, P, m) if n % 2 else None), n


# ---- 4: batches, jobs and repeated runs ---------------------------------------------------------------------------------------


def batch_groups():
    return [make_scalars(d, n, C_BIG, 40 + g) for g, (d, n, _) in enumerate(BATCH)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["w16", "tbl16x1"])
def test_batch_of_four_with_surplus_giants(ctx, big, mode):
    groups = batch_groups()
    offs = [off for _, _, off in BATCH]
    m = plan_model(groups, C_BIG, num_cus(), sets=mode_sets(mode))
    assert m["giants"] >= 2 * MAX_GIANTS, m["giants"]
    want = [o.msm_by_dlog_limbs(sc, big.curve, SEED_BIG, start=off) for sc, off in zip(groups, offs)]
    bases = big.plain if mode == "w16" else big.tbl1
    with window(ctx, C_BIG):
        got = ctx.msm_batch(bases, groups, offsets=offs)
    for g in range(len(groups)):
        assert aff(got[g], big.curve) == want[g], (mode, g, BATCH[g][0])


@pytest.mark.gpu
def test_job_of_the_same_four_groups(ctx, big):
    import torch
    groups = batch_groups()
    offs = [off for _, _, off in BATCH]
    want = [o.msm_by_dlog_limbs(sc, big.curve, SEED_BIG, start=off) for sc, off in zip(groups, offs)]
    dev = [torch.from_numpy(sc.view(np.int64)).cuda() for sc in groups]
    job = ctx.msm_job(big.tbl1, [len(sc) for sc in groups], offs)
    for g in (2, 0, 3, 1):
        job.push(g, dev[g])
    got = job.finish()
    for g in range(len(groups)):
        assert aff(got[g], big.curve) == want[g], (g, BATCH[g][0])


@pytest.mark.gpu
@pytest.mark.parametrize("serial", [1, 0], ids=["serial", "quad"])
def test_giant_state_between_runs(ctx, big, serial):
    """The giants' arrival counters and both queues are reset in pass A (k_part_scan): a surplus-giant run, another giant
    run, then the first again on one context, all exact."""
    runs = ["few64", "all_equal", "few64", "few2", "few64"]
    with tuned(fixup_serial=serial):
        for k, dist in enumerate(runs):
            sc, want = big.case(dist)
            for mode in ("w16", "tbl16x1"):
                assert run_mode(ctx, big, mode, sc) == want, (k, dist, mode)


# ---- 5: digit edges for every window -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", [4, 7, 11, 13, 16, 17, 19, 20])
@pytest.mark.parametrize("curve", CURVES, ids=["pallas", "vesta"])
def test_digit_edges_for_every_window(ctx, curve, c):
    n, seed = 3000, 0xED6E + c
    cases = [(d, make_scalars(d, n, c, c)) for d in ("top_digit", "top_digit1", "ones_carry")]
    assert plan_model([cases[0][1]], c, num_cus())["top_hits"] >= (n // 2) * (253 // c)
    assert plan_model([cases[2][1]], c, num_cus())["zero_signed"] >= n // 2
    want = {d: o.msm_by_dlog_limbs(sc, curve, seed) for d, sc in cases}
    bases = ctx.bases_generate(curve, seed, n)
    try:
        with window(ctx, c):
            for d, sc in cases:
                assert aff(ctx.msm(bases, sc), curve) == want[d], ("table-less", d)
            if c >= 8:
                bases.precompute(c, 1)
                for d, sc in cases:
                    assert aff(ctx.msm(bases, sc), curve) == want[d], ("table", d)
    finally:
        bases.free()
