"""GPU parity of the compression-SNARK building blocks (include/vdf_hip.h) against oracle/spartan.py, bit-exact."""
import functools

import numpy as np
import pytest

from oracle import pasta as o
from oracle import spartan as sp
from util import limbs, ints, mont, unmont, rand_limbs

pytestmark = pytest.mark.gpu
F, Q = o.FIELD_FQ, o.Q


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view("<u8")


def _rand(seed, n):
    return [o.rand_fe(seed, i, Q) for i in range(n)]


@pytest.mark.parametrize("k", [0, 1, 5, 11])
def test_pair_table_is_the_eq_table(ctx, k):
    r = _rand(k + 1, k)
    out = _dev(np.zeros((1 << k, 4), dtype="<u8"))
    ctx.pair_table(F, mont([(1 - x) % Q for x in r], Q) if k else None, mont(r, Q) if k else None, k, out)
    ctx.sync()
    assert unmont(_host(out), Q) == sp.eq_table(r, Q)


def test_fold_halves_binds_and_folds(ctx):
    n = 1 << 12
    vs = [_rand(10 + t, n) for t in range(3)]
    r, x = o.rand_fe(99, 0, Q), o.rand_fe(99, 1, Q)
    xi = pow(x, -1, Q)
    dv = [_dev(mont(v, Q)) for v in vs]
    ctx.fold_halves(F, dv, mont([(1 - r) % Q, x, xi], Q), mont([r, xi, x], Q), n)
    ctx.sync()
    h = n // 2
    assert unmont(_host(dv[0])[:h], Q) == sp.bind(vs[0], r, Q)
    assert unmont(_host(dv[1])[:h], Q) == [(vs[1][i] * x + vs[1][h + i] * xi) % Q for i in range(h)]
    assert unmont(_host(dv[2])[:h], Q) == [(vs[2][i] * xi + vs[2][h + i] * x) % Q for i in range(h)]
    assert unmont(_host(dv[2])[h:], Q) == vs[2][h:]                    # upper half untouched


@pytest.mark.parametrize("n", [2, 256, 1 << 13, 3 << 12])
def test_reductions(ctx, n):
    tabs = [_rand(20 + t, n) for t in range(5)]
    d = [_dev(mont(t, Q)) for t in tabs]
    u = o.rand_fe(5, 5, Q)
    assert unmont(ctx.reduce(F, 0, d[:2], n), Q) == [sum(a * b for a, b in zip(tabs[0], tabs[1])) % Q]
    if n & (n - 1):
        return                                                         # the round reductions need a power of two
    h = n // 2
    at = lambda f, i, t: (f[i] + t * (f[h + i] - f[i])) % Q
    quad = [sum(at(tabs[0], i, t) * at(tabs[1], i, t) for i in range(h)) % Q for t in (0, 2)]
    assert unmont(ctx.reduce(F, 1, d[:2], n), Q) == quad
    cubic = [sum(at(tabs[0], i, t) * ((at(tabs[1], i, t) * at(tabs[2], i, t) - u * at(tabs[3], i, t) - at(tabs[4], i, t)) % Q)
                 for i in range(h)) % Q for t in (0, 2, 3)]
    assert unmont(ctx.reduce(F, 2, d, n, u=mont([u], Q)), Q) == cubic
    cross = [sum(tabs[0][i] * tabs[1][h + i] for i in range(h)) % Q, sum(tabs[0][h + i] * tabs[1][i] for i in range(h)) % Q]
    assert unmont(ctx.reduce(F, 3, d[:2], n), Q) == cross


def _shape_arrays(entries):
    rows = np.array([e[0] for e in entries], dtype=np.uint32)
    cols = np.array([e[1] for e in entries], dtype=np.uint32)
    return rows, cols, mont([e[2] for e in entries], Q)


@pytest.mark.parametrize("t", [3, 64, 300])
def test_spmv3_transposed(ctx, t):
    """M(y) over the shape's own column order; t = 300 makes the constant column heavy (> 64 entries)."""
    sh = o.step_circuit_shape(t, F)
    ncols = sh.num_vars + 1 + sh.num_io
    shape = ctx.shape_create(F, sh.num_cons, ncols, [_shape_arrays(e) for e in (sh.A, sh.B, sh.C)])
    eq = _rand(t, sh.num_cons)
    rho = o.rand_fe(t, 777, Q)
    out = _dev(np.zeros((ncols, 4), dtype="<u8"))
    ctx.spmv3_t(shape, _dev(mont(eq, Q)), mont([rho], Q), out)
    ctx.sync()
    exp = [0] * ncols
    for coef, mat in ((1, sh.A), (rho, sh.B), (rho * rho % Q, sh.C)):
        for r, c, v in mat:
            exp[c] = (exp[c] + coef * v % Q * eq[r]) % Q
    assert unmont(_host(out), Q) == exp
    shape.free()


def test_ipa_round_helpers(ctx):
    n, nj = 1 << 10, 1 << 7
    a, s = _rand(1, nj), _rand(2, n)
    x = o.rand_fe(3, 0, Q)
    xi = pow(x, -1, Q)
    sL, sR = _dev(np.zeros((n, 4), dtype="<u8")), _dev(np.zeros((n, 4), dtype="<u8"))
    ds = _dev(mont(s, Q))
    ctx.ipa_scalars(F, _dev(mont(a, Q)), ds, n, nj, sL, sR)
    ctx.scale_pattern(F, ds, n, nj, mont([xi], Q), mont([x], Q))
    ctx.sync()
    h = nj // 2
    eL = [s[t] * a[(t % nj) - h] % Q if (t % nj) >= h else 0 for t in range(n)]
    eR = [s[t] * a[(t % nj) + h] % Q if (t % nj) < h else 0 for t in range(n)]
    assert unmont(_host(sL), Q) == eL and unmont(_host(sR), Q) == eR
    assert unmont(_host(ds), Q) == [s[t] * (x if (t % nj) >= h else xi) % Q for t in range(n)]


def test_building_blocks_in_the_other_field(ctx):
    """The same kernels instantiated for Fp (a Vesta-side argument would use them)."""
    Fp, P = o.FIELD_FP, o.P
    r = [o.rand_fe(7, i, P) for i in range(6)]
    out = _dev(np.zeros((64, 4), dtype="<u8"))
    ctx.pair_table(Fp, mont([(1 - x) % P for x in r], P), mont(r, P), 6, out)
    ctx.sync()
    assert unmont(_host(out), P) == sp.eq_table(r, P)
    a, b = [o.rand_fe(8, i, P) for i in range(64)], [o.rand_fe(9, i, P) for i in range(64)]
    da, db = _dev(mont(a, P)), _dev(mont(b, P))
    assert unmont(ctx.reduce(Fp, 0, [da, db], 64), P) == [sum(x * y for x, y in zip(a, b)) % P]
    assert unmont(ctx.reduce(Fp, 3, [da, db], 64), P) == [sum(a[i] * b[32 + i] for i in range(32)) % P,
                                                           sum(a[32 + i] * b[i] for i in range(32)) % P]
    ctx.fold_halves(Fp, [da], mont([(1 - r[0]) % P], P), mont([r[0]], P), 64)
    ctx.sync()
    assert unmont(_host(da)[:32], P) == sp.bind(a, r[0], P)


def test_scalar_and_vector_placement_is_checked(ctx):
    v = _dev(np.zeros((8, 4), dtype="<u8"))
    one = mont([1], Q)
    with pytest.raises(Exception):
        ctx.pair_table(F, _dev(one), _dev(one), 1, v)                 # scalars must be host memory
    with pytest.raises(Exception):
        ctx.fold_halves(F, [np.zeros((8, 4), dtype="<u8")], one, one, 8)      # vectors must be device memory
    with pytest.raises(Exception):
        ctx.fold_halves(F, [v], one, one, 6)                          # power of two


@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("k,log_m", [(0, 0), (0, 4), (3, 2), (9, 4), (14, 4)])
def test_pair_table_pattern(ctx, field, k, log_m):
    """out[i] = (pair table over the top k bits of i) * pattern[low log_m bits of i]."""
    import torch
    m = o.modulus(field)
    rng = np.random.default_rng(100 * k + log_m)
    lo, hi = [int(x) % m for x in ints(rand_limbs(rng, max(k, 1)))], [int(x) % m for x in ints(rand_limbs(rng, max(k, 1)))]
    pat = [int(x) % m for x in ints(rand_limbs(rng, 1 << log_m))]
    n = 1 << (k + log_m)
    out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    ctx.pair_table_pattern(field, mont(lo, m), mont(hi, m), k, mont(pat, m), log_m, out)
    ctx.sync()
    got = unmont(out.cpu().numpy().view("<u8"), m)
    idx = sorted(i for i in set([0, 1, n - 1, n // 2, n // 3] + [int(x) for x in rng.integers(0, n, size=40)]) if i < n)
    for i in idx:
        e = pat[i & ((1 << log_m) - 1)]
        top = i >> log_m
        for j in range(k):
            e = e * (hi[j] if (top >> (k - 1 - j)) & 1 else lo[j]) % m
        assert got[i] == e, i
    with pytest.raises(Exception):
        ctx.pair_table_pattern(field, mont(lo, m), mont(hi, m), k, mont(pat + [1] * 16, m), 5, out)      # pattern too long


# ---- every size regime of the blocks, against big-integer formulas over the tests' own inputs ------------------------------------
FIELDS = [o.FIELD_FP, o.FIELD_FQ]
ONES = 0xFFFFFFFFFFFFFFFF                                               # prefill of an output: an unwritten element shows up


def _randm(rng, m, k):
    return [int(x) % m for x in ints(rand_limbs(rng, k))]


# -- vdf_spmv3_t over skewed columns: <= 64 entries a thread, 65..4096 a workgroup, more than 4096 shared by 64 workgroups as far
# -- as the 48 KB scratch holds their partials (24 columns; 24 / 12 / 6 for the batch widths 1 / 2 / 4), the rest one workgroup each
SKEWED_CONS = 6144
FEW_BIG = [0, 1, 2, 63, 64, 65, 66, 127, 255, 256, 257, 511, 1000, 4095, 4096, 4097, 4160, 4161, 8191, 12000]
SKEWED_PROFILES = {"few-big": FEW_BIG,                                  # 5 columns past 4096: within the scratch at every width
                   "many-big": FEW_BIG + list(range(4100, 4131))}       # 36 of them: past the room of 24, 12 and 6
SKEWED_DUPLICATES = {66: 2, 4097: 3, 12000: 2}                          # column length -> repeated (row, column) pairs inside A


@functools.lru_cache(maxsize=None)
def skewed_shape(profile, field):
    """(mats, triples, ncols): the COO arrays for shape_create and the same triples as (rows, cols, coefficient integers).  Column
    c has SKEWED_PROFILES[profile][c] entries, a third in each of A, B, C, on random distinct rows of a matrix (but for the
    deliberate duplicates, which are legal COO and sum); column 0 is empty and the last column is one of the longest, so
    colptr[c + 1] is read at the end of the array.  Coefficients come from a pool of 53 values with +1, -1 and 2 in it, and the
    triples are handed over in shuffled order."""
    m = o.modulus(field)
    lens = SKEWED_PROFILES[profile]
    rng = np.random.default_rng(4000 + 10 * len(lens) + field)
    pool = [1, m - 1, 2] + _randm(rng, m, 50)
    pool_mont, pool_obj = mont(pool, m), np.array(pool, dtype=object)
    mats, triples = [], []
    for k in range(3):
        rows, cols = [], []
        for c, ln in enumerate(lens):
            part = ln // 3 + (1 if k < ln % 3 else 0)
            dup = SKEWED_DUPLICATES.get(ln, 0) if k == 0 else 0
            r = rng.choice(SKEWED_CONS, part - dup, replace=False)
            rows.append(np.concatenate([r, r[:dup]]))
            cols.append(np.full(part, c))
        rows, cols = np.concatenate(rows).astype(np.uint32), np.concatenate(cols).astype(np.uint32)
        order = rng.permutation(rows.size)
        rows, cols = rows[order], cols[order]
        ci = rng.integers(0, len(pool), size=rows.size)
        mats.append((rows, cols, np.ascontiguousarray(pool_mont[ci])))
        triples.append((rows, cols, pool_obj[ci]))
    got_lens = sum(np.bincount(t[1], minlength=len(lens)) for t in triples)
    assert got_lens.tolist() == lens and len(set(zip(triples[0][0].tolist(), triples[0][1].tolist()))) == triples[0][0].size - 7
    return mats, triples, len(lens)


def skewed_eq(rng, m):
    eq = _randm(rng, m, SKEWED_CONS)
    for r in rng.choice(SKEWED_CONS, 200, replace=False):
        eq[int(r)] = 0
    for r in rng.choice(SKEWED_CONS, 200, replace=False):
        eq[int(r)] = m - 1
    return eq


def spmvt_formula(triples, eq, rho, ncols, m):
    """exp[c] = sum over the triples (row, c, val) of coef * val * eq[row], coef = 1, rho, rho^2 for A, B, C"""
    eq = np.array(eq, dtype=object)
    exp = [0] * ncols
    for coef, (rows, cols, vals) in zip((1, rho, rho * rho % m), triples):
        term = vals * eq[rows]
        for c in range(ncols):
            exp[c] = (exp[c] + coef * int(term[cols == c].sum())) % m
    return exp


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("profile", ["few-big", "many-big"])
def test_spmv3_transposed_skewed_columns(ctx, profile, field):
    """few-big: k_spmvt, k_spmvt_heavy and k_spmvt_heavy_part / k_spmvt_heavy_sum (chunks of 65, 65, 66, 128 and 188 entries per
    part, the last parts short or empty); many-big: 36 columns past 4096 entries, 12 of them past the scratch's room of 24 and so
    launched from heavy + shared."""
    m = o.modulus(field)
    mats, triples, ncols = skewed_shape(profile, field)
    shape = ctx.shape_create(field, SKEWED_CONS, ncols, mats)
    rng = np.random.default_rng(17 + field + ncols)
    eq = skewed_eq(rng, m)
    for rho in _randm(rng, m, 1) + [0, 1]:
        out = _dev(np.full((ncols, 4), ONES, dtype="<u8"))
        ctx.spmv3_t(shape, _dev(mont(eq, m)), mont([rho], m), out)
        ctx.sync()
        exp = spmvt_formula(triples, eq, rho, ncols, m)
        assert exp[0] == 0 and ints(_host(out)) == ints(mont(exp, m)), rho
    shape.free()


# -- vdf_reduce past the grid cap of 512 workgroups (h > 131072: k_reduce strides) and past 256 partials (h > 65536: the final
# -- pass takes several per lane)
BIG_N = 1 << 19


@functools.lru_cache(maxsize=None)
def big_reduction(field):
    """Five tables of 2^19 raw canonical residues (below 2^254 < m), a residue u, and what each reduction returns over them.
    The device multiplies residues by Montgomery's product x * y -> x y R^-1 mod m and adds, subtracts and doubles them as they
    are, so the returned residue is a closed form in the raw integers with one R^-1 per product, computed here once per field:
      ("dot", n, i, j)   kind 0 over the first n elements of tables i and j
      (kind, BIG_N)      kinds 1, 2, 3 over the whole tables"""
    m = o.modulus(field)
    rng = np.random.default_rng(900 + field)
    tabs = [rand_limbs(rng, BIG_N) for _ in range(5)]
    u_limbs = rand_limbs(rng, 1)
    T = [np.array(ints(t), dtype=object) for t in tabs]
    u, ri = ints(u_limbs)[0], pow(o.R, -1, m)
    exp = {}
    # kind 0: out = R^-1 * sum a[i] b[i]
    prod = [T[j] * T[j + 1] for j in range(3)]
    for n in (BIG_N, 65537, 131329):
        exp["dot", n, 0, 1] = [ri * int(prod[0][:n].sum()) % m]
    for j in range(3):
        exp["dot", 1 << 18, j, j + 1] = [ri * int(prod[j][:1 << 18].sum()) % m]
    del prod
    h = BIG_N // 2
    lo, d = [t[:h] for t in T], [t[h:] - t[:h] for t in T]
    at = lambda k, t: lo[k] + t * d[k]                                  # the table bound to t, as an integer congruent to the device's
    # kind 1: out[t] = R^-1 * sum p_t[i] q_t[i], t = 0, 2
    exp[1, BIG_N] = [ri * int((at(0, t) * at(1, t)).sum()) % m for t in (0, 2)]
    # kind 2: out[t] = R^-1 * sum eq_t[i] * (R^-1 * (a_t[i] b_t[i] - u c_t[i]) - e_t[i]), t = 0, 2, 3: the products a b and u c carry
    # one R^-1, the outer product by eq a second one
    exp[2, BIG_N] = [ri * int((at(0, t) * (ri * (at(1, t) * at(2, t) - u * at(3, t)) % m - at(4, t))).sum()) % m for t in (0, 2, 3)]
    # kind 3: out = R^-1 * sum a[i] b[h + i],  R^-1 * sum a[h + i] b[i]
    exp[3, BIG_N] = [ri * int((T[0][:h] * T[1][h:]).sum()) % m, ri * int((T[0][h:] * T[1][:h]).sum()) % m]
    return tabs, u_limbs, exp


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_reductions_above_the_grid_cap(ctx, field, kind):
    """n = 2^19: h = 2^18 for the rounds (512 workgroups of two strides each, 512 partials: two per lane of the final pass), and
    four strides for the dot product."""
    tabs, u, exp = big_reduction(field)
    d = [_dev(t) for t in tabs[:5 if kind == 2 else 2]]
    got = ctx.reduce(field, kind, d, BIG_N, u=u if kind == 2 else None)
    assert ints(got) == (exp["dot", BIG_N, 0, 1] if kind == 0 else exp[kind, BIG_N])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [65537, 131329])
def test_dot_product_at_the_stride_and_partial_edges(ctx, field, n):
    """65537: 257 partials, the first lane of the final pass takes a second one; 131329: 514 workgroups' worth on a grid of 512,
    so only workgroups 0 and 1 stride, the second one with a single lane."""
    tabs, _, exp = big_reduction(field)
    got = ctx.reduce(field, 0, [_dev(tabs[0][:n]), _dev(tabs[1][:n])], n)
    assert ints(got) == exp["dot", n, 0, 1]


# -- vdf_ipa_scalars / vdf_scale_pattern at the edges of n_j: 2 (h = 1), n (no wrap), n below one workgroup
def _ipa_helpers(ctx, field, n, nj, seed):
    m = o.modulus(field)
    rng = np.random.default_rng(seed)
    a, s = _randm(rng, m, nj), _randm(rng, m, n)
    x, = _randm(rng, m, 1)
    xi = pow(x, -1, m)
    sL, sR = _dev(np.full((n, 4), ONES, dtype="<u8")), _dev(np.full((n, 4), ONES, dtype="<u8"))
    ds = _dev(mont(s, m))
    da = _dev(np.concatenate([mont(a, m), np.full((1, 4), ONES, dtype="<u8")]))     # a sentinel past a's n_j elements: never read
    ctx.ipa_scalars(field, da, ds, n, nj, sL, sR)
    ctx.scale_pattern(field, ds, n, nj, mont([xi], m), mont([x], m))
    ctx.sync()
    h = nj // 2
    eL = [s[t] * a[(t % nj) - h] % m if (t % nj) >= h else 0 for t in range(n)]
    eR = [s[t] * a[(t % nj) + h] % m if (t % nj) < h else 0 for t in range(n)]
    assert ints(_host(sL)) == ints(mont(eL, m)) and ints(_host(sR)) == ints(mont(eR, m))
    assert ints(_host(ds)) == ints(mont([s[t] * (x if (t % nj) >= h else xi) % m for t in range(n)], m))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n,nj", [(2, 2), (64, 2), (64, 64), (4096, 2), (4096, 4096), (1 << 13, 256)])
def test_ipa_round_helpers_at_the_edges(ctx, field, n, nj):
    _ipa_helpers(ctx, field, n, nj, 3 * n + nj + field)


@pytest.mark.parametrize("field", FIELDS)
def test_ipa_round_helpers_refuse_bad_lengths(ctx, field):
    m = o.modulus(field)
    rng = np.random.default_rng(60 + field)
    bufs = [rand_limbs(rng, 1024) for _ in range(4)]
    da, ds, sL, sR = (_dev(b) for b in bufs)
    x = mont([3], m)
    for n, nj in [(1024, 0), (1024, 1), (64, 128), (64, 6), (6, 2), (0, 2)]:
        with pytest.raises(Exception):
            ctx.ipa_scalars(field, da, ds, n, nj, sL, sR)
        with pytest.raises(Exception):
            ctx.scale_pattern(field, ds, n, nj, x, x)
        ctx.sync()
        for dv, b in zip((da, ds, sL, sR), bufs):
            assert np.array_equal(_host(dv), b), (n, nj)


# -- vdf_pair_table at depth: the variable-to-bit order at every index bit
@pytest.mark.parametrize("field", FIELDS)
def test_pair_table_k18_is_the_eq_table(ctx, field):
    m, k = o.modulus(field), 18
    r = _randm(np.random.default_rng(180 + field), m, k)
    out = _dev(np.full((1 << k, 4), ONES, dtype="<u8"))
    ctx.pair_table(field, mont([(1 - x) % m for x in r], m), mont(r, m), k, out)
    ctx.sync()
    assert ints(_host(out)) == ints(mont(sp.eq_table(r, m), m))


@pytest.mark.parametrize("field", FIELDS)
def test_pair_table_k22_samples(ctx, field):
    """128 MB of table, sampled: both ends, every index of a single set bit and of a single clear bit (variable j is bit k-1-j, so
    each of these pins one variable's position), and 64 random indices."""
    import torch
    m, k = o.modulus(field), 22
    n = 1 << k
    rng = np.random.default_rng(220 + field)
    lo, hi = _randm(rng, m, k), _randm(rng, m, k)
    idx = [0, n - 1] + [1 << b for b in range(k)] + [n - 1 - (1 << b) for b in range(k)] + [int(i) for i in rng.integers(0, n, size=64)]
    out = torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
    ctx.pair_table(field, mont(lo, m), mont(hi, m), k, out)
    ctx.sync()
    got = unmont(_host(out[torch.tensor(idx, device="cuda")]), m)
    for i, g in zip(idx, got):
        e = 1
        for j in range(k):
            e = e * (hi[j] if (i >> (k - 1 - j)) & 1 else lo[j]) % m
        assert g == e, i


def test_pair_table_refuses_25_variables(ctx):
    c = mont([1] * 25, Q)
    with pytest.raises(Exception):
        ctx.pair_table(F, c, c, 25, _dev(np.zeros((8, 4), dtype="<u8")))
