"""The device field and curve primitives (vdf_amd/csrc/fe.cuh, ec.cuh) as plain Python integers, with the case generators
of tests/test_prim_spec.py and tests/test_gpu_primitives.py.  No device, no ctypes; oracle/pasta.py supplies the moduli, the
Montgomery maps and the affine group law only.  Every operation has ONE right answer as a 256-bit integer, so every
comparison against tools/ubench/prim_check is an equality.

The lazy domain and the slack invariant
---------------------------------------
m = 2^254 + c (c < 2^126), R = 2^256, redc(T) = (T + q m) / R with q = -T / m mod R < R, so redc(T) <= (T + (R - 1) m) / R.
eps = ceil(m (m - 2^254) / 2^254) ~ 2^125.1.  A lazy value "has slack d" when it is below 2m + d.

  product   a <= A, b <= B:  redc(ab) <= (A B + (R - 1) m) >> 256.  With A = 2m + da, B = 2m + db this is
            m + m^2 / 2^254 + (da + db) m / 2^255 + da db / R = 2m + eps + (da + db) / 2 (1 + 2^-128) + da db / R: slack
            eps + half the factors' slacks (the two tails are below 2 for slacks of a few eps; the floor absorbs them --
            `closes()` below evaluates the bound in exact integers instead of trusting this sentence).  A canonical factor
            (< m) gives a product below 1.5 m + ...: below 2m, slack 0.
  pair      redc(ab + cd) <= (A B + C D + (R - 1) m) >> 256 must stay below 2^256 (the ninth word of the column scan);
            then t >= 2^255 -> t - m, so the result is at most max(2^255 - 1, t_max - m): slack 2 eps + half of all four.
  a - b     (+ 2m on borrow): at most max(A, 2m - 1), the MINUEND's slack.  PRECONDITION b <= a + 2m: for b > a + 2m the
            corrected difference is still negative and wraps.  A subtrahend with slack d violates it only when the minuend is
            below d, i.e. for a fraction d / m < 2^-126 of uniformly distributed minuends (ec.cuh states this; the model
            below raises on it, and the generators emit no such state).

One xyzz_madd_lazy step on a state with X < 2m + eps, Y < 2m + 9 eps, ZZ < 2m + 4 eps, ZZZ < 2m + 4.5 eps and canonical b:
  U2 = x_b ZZ, S2 = y_b ZZZ < 2m (canonical factor);  P' = X - U2 <= max(X, 2m - 1): slack eps;  R = S2 - Y < 2m: slack 0
  PP = P'^2: 2 eps;  PPP' = P' PP: 2.5 eps;  Q = X PP: 2.5 eps;  R^2: eps;  X3 = (R^2 - Q) - (Q - PPP'): minuend R^2: eps
  Y3 = pair(R, Q - X3, Y, PPP') : 2 eps + (0 + 2.5 + 9 + 2.5) / 2 eps = 9 eps          (fixed point of d = 4.5 eps + d / 2)
  ZZ3 = ZZ PP: eps + (4 + 2) / 2 eps = 4 eps;  ZZZ3 = ZZZ PPP': eps + (4.5 + 2.5) / 2 eps = 4.5 eps
so (eps, 9 eps, 4 eps, 4.5 eps) maps into itself: ec.cuh's figures are right, and all below 2m + 9 eps.  The doubling branch
stores canonical coordinates.  xyzz_add_lazy with canonical b: U1, U2, S1, S2 < 2m, so P', R < 2m and X3 has slack eps,
Y3 <= 2^255 - 1 < 2m, ZZ3, ZZZ3 < 2m (a product of a product with a canonical factor): every state below 2m + 4 eps -- and
every madd state too -- goes to a state below 2m + 4 eps, as ec.cuh says (in fact below 2m + eps).  Both statements are checked
in exact integer interval arithmetic by `closes()`.

In xyzz_add_lazy U1 and U2 are both below 1.5 m + ..., so P' = U1 - U2 (+ 2m) is never 2m: of the three values the
`v[0] <= 2` filter admits only 0 and m are reachable there; in xyzz_madd_lazy all three are (X = U2 + 2m needs U2 < eps)."""
import random
from fractions import Fraction

from oracle import pasta as o

R = 1 << 256
MASK = R - 1
FP, FQ = 0, 1


class Field:
    def __init__(self, fid, name, m, curve):
        self.fid, self.name, self.m, self.curve = fid, name, m, curve
        self.nminv = (-pow(m, -1, R)) % R
        self.c = m - (1 << 254)
        self.eps = -((-m * self.c) >> 254)
        self.one = R % m
        self.r2 = R * R % m

    def __repr__(self):
        return self.name


FIELDS = (Field(FP, "fp", o.P, o.CURVE_PALLAS), Field(FQ, "fq", o.Q, o.CURVE_VESTA))

# slack of a stored accumulator in half-eps units: (x, y, zz, zzz)
MADD_SLACK2 = (2, 18, 8, 9)
ADD_SLACK2 = (8, 8, 8, 8)


def limit(F, k2):
    """exclusive upper bound 2m + (k2 / 2) eps of a coordinate with slack k2 half-eps (rounded down)"""
    return 2 * F.m + k2 * F.eps // 2


def lazy_top(F):
    return limit(F, 18)                                   # the contract of every lazy operand: below 2m + 9 eps


def inside(F, acc, slack2):
    return all(0 <= v < limit(F, k) for v, k in zip(acc, slack2))


# ---- field operations ------------------------------------------------------------------------------------------------
def redc(F, T):
    q = (T * F.nminv) & MASK
    s = T + q * F.m
    assert s & MASK == 0
    return s >> 256


def fe_mul_lazy(F, a, b):
    return redc(F, a * b)


def fe_sqr_lazy(F, a):
    return redc(F, a * a)


def _csub(F, a):
    return a - F.m if a >= F.m else a


def fe_mul_inl(F, a, b):
    return _csub(F, redc(F, a * b))


def fe_sqr_inl(F, a):
    return _csub(F, redc(F, a * a))


def fe_mul2_lazy(F, a, b, c, d):
    t = redc(F, a * b + c * d)
    if t >= R:
        raise ValueError("fe_mul2_lazy: the column scan needs a ninth word")
    return t - F.m if t >= 1 << 255 else t


def fe_sub_lazy(F, a, b):
    r = a - b if a >= b else a - b + 2 * F.m
    if r < 0:
        raise ValueError("fe_sub_lazy: b > a + 2m")
    return r


def fe_neg_lazy(F, a):
    if a > 3 * F.m:
        raise ValueError("fe_neg_lazy: a > 3m")
    return 3 * F.m - a


def fe_neg_nz(F, a):
    return F.m - a


def fe_canon(F, a):
    return _csub(F, _csub(F, a))


def fe_add(F, a, b):
    return (a + b) % F.m


def fe_sub(F, a, b):
    return (a - b) % F.m


def fe_neg(F, a):
    return (-a) % F.m


def fe_dbl(F, a):
    return 2 * a % F.m


def fe_from_small(F, k):
    return k * R % F.m


def fe_from_small_went_negative(F, k):
    """whether fe.cuh's fe_from_small takes its `add m` branch for k: x = k (R mod m), q = x >> 254, (x mod 2^254) < q c"""
    x = k * F.one
    return (x & ((1 << 254) - 1)) < (x >> 254) * F.c


def fe_from_mont(F, a):
    return o.from_mont(a, F.m)


def fe_to_mont(F, a):
    return o.to_mont(a, F.m)


def fe_inv(F, a):
    """Montgomery form in, Montgomery form out: (a / R)^(m - 2) R"""
    return o.to_mont(pow(o.from_mont(a, F.m), F.m - 2, F.m), F.m)


def fe_is_canonical(F, a):
    return int(a < F.m)


# ---- canonical XYZZ law (what the exceptional branches of the lazy additions call), Montgomery residues ----------------
def _cm(F, a, b):
    return fe_mul_inl(F, a, b)


def xyzz_dbl_affine(F, b):
    x, y = b
    U = fe_dbl(F, y); V = _cm(F, U, U); W = _cm(F, U, V); S = _cm(F, x, V); X2 = _cm(F, x, x)
    M = fe_add(F, fe_dbl(F, X2), X2)
    x3 = fe_sub(F, fe_sub(F, _cm(F, M, M), S), S)
    y3 = fe_sub(F, _cm(F, M, fe_sub(F, S, x3)), _cm(F, W, y))
    return (x3, y3, V, W)


def xyzz_dbl(F, a):
    if a[2] == 0:
        return a
    x, y, zz, zzz = a
    x3, y3, V, W = xyzz_dbl_affine(F, (x, y))
    return (x3, y3, _cm(F, V, zz), _cm(F, W, zzz))


def xyzz_add(F, a, b):
    if b[2] == 0:
        return a
    if a[2] == 0:
        return b
    U1 = _cm(F, a[0], b[2]); U2 = _cm(F, b[0], a[2]); S1 = _cm(F, a[1], b[3]); S2 = _cm(F, b[1], a[3])
    Pp, Rr = fe_sub(F, U2, U1), fe_sub(F, S2, S1)
    if Pp == 0:
        return xyzz_dbl(F, a) if Rr == 0 else (0, 0, 0, 0)
    PP = _cm(F, Pp, Pp); PPP = _cm(F, Pp, PP); Q = _cm(F, U1, PP)
    x3 = fe_sub(F, fe_sub(F, fe_sub(F, _cm(F, Rr, Rr), PPP), Q), Q)
    y3 = fe_sub(F, _cm(F, Rr, fe_sub(F, Q, x3)), _cm(F, S1, PPP))
    return (x3, y3, _cm(F, _cm(F, a[2], b[2]), PP), _cm(F, _cm(F, a[3], b[3]), PPP))


# ---- the lazy additions, from the formulas in ec.cuh's comment ----------------------------------------------------------
def _same_x(F, Pn):
    return (Pn & 0xFFFFFFFF) <= 2 and fe_canon(F, Pn) == 0


def xyzz_madd_lazy(F, acc, have, flip, b):
    """-> (acc, have, flip, P') ; P' is None on the first branch"""
    if not have:
        return (b[0], b[1], F.one, F.one), 1, 0, None
    x, y, zz, zzz = acc
    U2, S2 = fe_mul_lazy(F, b[0], zz), fe_mul_lazy(F, b[1], zzz)
    Pn, Rr = fe_sub_lazy(F, x, U2), fe_sub_lazy(F, S2, y)
    if _same_x(F, Pn):
        if fe_canon(F, Rr) == 0:
            return xyzz_dbl_affine(F, b), have, flip, Pn
        return acc, 0, flip, Pn
    PP = fe_sqr_lazy(F, Pn); PPPn = fe_mul_lazy(F, Pn, PP); Q = fe_mul_lazy(F, x, PP)
    X3 = fe_sub_lazy(F, fe_sub_lazy(F, fe_sqr_lazy(F, Rr), Q), fe_sub_lazy(F, Q, PPPn))
    Y3 = fe_mul2_lazy(F, Rr, fe_sub_lazy(F, Q, X3), y, PPPn)
    return (X3, Y3, fe_mul_lazy(F, zz, PP), fe_mul_lazy(F, zzz, PPPn)), 1, flip ^ 1, Pn


def xyzz_lazy_resolve(F, acc, have, flip):
    if not have:
        return (0, 0, 0, 0)
    return (acc[0], fe_neg_lazy(F, acc[1]) if flip else acc[1], acc[2], acc[3])


def xyzz_add_lazy(F, acc, have, flip, b):
    if not have:
        return tuple(b), 1, 0, None
    U1, U2 = fe_mul_lazy(F, acc[0], b[2]), fe_mul_lazy(F, b[0], acc[2])
    S1, S2 = fe_mul_lazy(F, acc[1], b[3]), fe_mul_lazy(F, b[1], acc[3])
    Pn, Rr = fe_sub_lazy(F, U1, U2), fe_sub_lazy(F, S2, S1)
    if _same_x(F, Pn):
        a = tuple(fe_canon(F, v) for v in xyzz_lazy_resolve(F, acc, have, flip))
        bb = (b[0], fe_neg(F, b[1]) if flip else b[1], b[2], b[3])
        r = xyzz_add(F, a, bb)
        return r, int(r[2] != 0), 0, Pn
    PP = fe_sqr_lazy(F, Pn); PPPn = fe_mul_lazy(F, Pn, PP); Q = fe_mul_lazy(F, U1, PP)
    X3 = fe_sub_lazy(F, fe_sub_lazy(F, fe_sqr_lazy(F, Rr), Q), fe_sub_lazy(F, Q, PPPn))
    Y3 = fe_mul2_lazy(F, Rr, fe_sub_lazy(F, Q, X3), S1, PPPn)
    return (X3, Y3, fe_mul_lazy(F, fe_mul_lazy(F, acc[2], b[2]), PP), fe_mul_lazy(F, fe_mul_lazy(F, acc[3], b[3]), PPPn)), 1, flip ^ 1, Pn


def closes(F):
    """The invariant in exact interval arithmetic (inclusive maxima): madd maps MADD_SLACK2 into itself, add maps both
    ADD_SLACK2 and MADD_SLACK2 into ADD_SLACK2, the pair never needs a ninth word, U1 - U2 + 2m < 2m in add."""
    m = F.m
    U = lambda A, B: (A * B + (R - 1) * m) >> 256
    lo2 = 2 * m - 1

    def pair(A, B, C, D):
        t = (A * B + C * D + (R - 1) * m) >> 256
        assert t < R
        return max((1 << 255) - 1, t - m)

    def madd(bx, by, bz, bw):
        assert U(m - 1, bz) < 2 * m and U(m - 1, bw) < 2 * m
        pn, rr = max(bx, lo2), lo2
        pp = U(pn, pn); ppp = U(pn, pp); q = U(bx, pp)
        x3 = max(U(rr, rr), lo2)
        return x3, pair(rr, max(q, lo2), by, ppp), U(bz, pp), U(bw, ppp)

    def add(bx, by, bz, bw):
        u1, u2, s1, s2 = U(bx, m - 1), U(m - 1, bz), U(by, m - 1), U(m - 1, bw)
        assert max(u1, u2, s1, s2) < 2 * m                 # so P' = U1 - U2 (+ 2m) is below 2m: never exactly 2m
        pn = rr = lo2
        pp = U(pn, pn); ppp = U(pn, pp); q = U(u1, pp)
        return max(U(rr, rr), lo2), pair(rr, max(q, lo2), s1, ppp), U(U(bz, m - 1), pp), U(U(bw, m - 1), ppp)

    top = lambda s2: tuple(limit(F, k) - 1 for k in s2)
    ok = all(v <= t for v, t in zip(madd(*top(MADD_SLACK2)), top(MADD_SLACK2)))
    ok = ok and all(v <= t for v, t in zip(add(*top(ADD_SLACK2)), top(ADD_SLACK2)))
    ok = ok and all(v <= t for v, t in zip(add(*top(MADD_SLACK2)), top(ADD_SLACK2)))
    ok = ok and all(v <= t for v, t in zip(madd(*add(*top(ADD_SLACK2))), top(MADD_SLACK2)))     # add's output may enter madd
    return ok and lazy_top(F) < R and 3 * m < R


# ---- affine points <-> stored accumulators -------------------------------------------------------------------------------
def affine_mont(F, pt):
    """oracle point (plain integers, None = identity) -> the device's affine encoding in Montgomery residues"""
    return (0, 0) if pt is None else (o.to_mont(pt[0], F.m), o.to_mont(pt[1], F.m))


def xyzz_mont(F, pt, z):
    """canonical XYZZ coordinates of `pt` with zz = z^2, zzz = z^3 (plain z != 0)"""
    if pt is None:
        return (0, 0, 0, 0)
    m = F.m
    return tuple(o.to_mont(v, m) for v in (pt[0] * z * z, pt[1] * z * z * z, z * z, z * z * z))


def xyzz_point(F, acc):
    """any representatives of XYZZ Montgomery coordinates -> oracle point"""
    m = F.m
    x, y, zz, zzz = (o.from_mont(v % m, m) for v in acc)
    if zz == 0:
        return None
    return (x * pow(zz, -1, m) % m, y * pow(zzz, -1, m) % m)


def jac_point(F, j):
    m = F.m
    x, y, z = (o.from_mont(v % m, m) for v in j)
    if z == 0:
        return None
    zi = pow(z, -1, m)
    return (x * zi * zi % m, y * zi * zi * zi % m)


def affine_point(F, a):
    m = F.m
    return None if a[0] % m == 0 and a[1] % m == 0 else (o.from_mont(a[0] % m, m), o.from_mont(a[1] % m, m))


def mul_g(F, k):
    return o.pt_mul(k, o.generator(F.curve), F.m)


# ---- operand lists -------------------------------------------------------------------------------------------------------
def edge_values(F, rng):
    m, e = F.m, F.eps
    v = [0, 1, 2, m - 2, m - 1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1,
         (1 << 254) - 1, 1 << 254, (1 << 255) - 1, 1 << 255, (1 << 255) + 1,
         2 * m + e - 1, 2 * m + 9 * e - 1, 3 * m - 1, 3 * m, F.c, F.one, F.r2]
    v += [0xFFFFFFFF << (32 * i) for i in range(8)]
    v.append(sum(0x80000000 << (32 * i) for i in range(8)))
    for lo in (0, 1, 2):
        for top in (m, 2 * m, lazy_top(F)):
            v.append(((rng.randrange(top) >> 32) << 32) | lo)
    return v


def random_values(F, rng, n, top=None):
    """n values from [0, m), [m, 2m) and [2m, 2m + 9 eps) in turn (only the ranges below `top`)"""
    m = F.m
    ranges = [(0, m), (m, 2 * m), (2 * m, lazy_top(F))]
    ranges = [r for r in ranges if top is None or r[1] <= top]
    return [rng.randrange(*ranges[i % len(ranges)]) for i in range(n)]


N_RANDOM = 4096
# op name -> (arity, exclusive operand bound as a function of the field, extra precondition on the operand tuple)
_nz = lambda F, t: t[0] % F.m != 0
_sub_ok = lambda F, t: t[1] <= t[0] + 2 * F.m
FIELD_OPS = {
    "fe_mul_lazy": (2, lazy_top, None), "fe_sqr_lazy": (1, lazy_top, None),
    "fe_mul_inl": (2, lambda F: F.m, None), "fe_sqr_inl": (1, lambda F: F.m, None), "fe_mul": (2, lambda F: F.m, None),
    "fe_mul2_lazy": (4, lazy_top, None), "fe_sub_lazy": (2, lazy_top, _sub_ok),
    "fe_neg_lazy": (1, lambda F: 3 * F.m + 1, _nz), "fe_neg_nz": (1, lambda F: F.m, _nz),
    "fe_canon": (1, lambda F: 3 * F.m + 1, None),
    "fe_add": (2, lambda F: F.m, None), "fe_sub": (2, lambda F: F.m, None), "fe_neg": (1, lambda F: F.m, None),
    "fe_dbl": (1, lambda F: F.m, None), "fe_from_mont": (1, lambda F: F.m, None), "fe_to_mont": (1, lambda F: F.m, None),
    "fe_inv": (1, lambda F: F.m, None), "fe_is_canonical": (1, lambda F: R, None),
}
FIELD_MODEL = {
    "fe_mul_lazy": fe_mul_lazy, "fe_sqr_lazy": fe_sqr_lazy, "fe_mul_inl": fe_mul_inl, "fe_sqr_inl": fe_sqr_inl, "fe_mul": fe_mul_inl,
    "fe_mul2_lazy": fe_mul2_lazy, "fe_sub_lazy": fe_sub_lazy, "fe_neg_lazy": fe_neg_lazy, "fe_neg_nz": fe_neg_nz, "fe_canon": fe_canon,
    "fe_add": fe_add, "fe_sub": fe_sub, "fe_neg": fe_neg, "fe_dbl": fe_dbl, "fe_from_mont": fe_from_mont, "fe_to_mont": fe_to_mont,
    "fe_inv": fe_inv, "fe_is_canonical": fe_is_canonical, "fe_from_small": fe_from_small,
}
# fe_canon's contract is [0, 2m + eps); it is also what brings fe_neg_lazy's (m - 9 eps, 3m) home, so it is driven up to 3m - 1
# (3m itself, the image of a = 0, is the documented exception: it stays at m).


def field_cases(F, op, seed=1, n_random=N_RANDOM):
    """operand tuples of a field op: the edge list (restricted to the op's contract) crossed with itself for binary ops, edge
    tuples for the four-operand pair, then n_random random tuples over the ranges the contract allows"""
    rng = random.Random((seed << 8) | F.fid)
    if op == "fe_from_small":
        ks = [0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 65535, 65536, (1 << 30) - 1, (1 << 30) - 2, 1 << 29, (1 << 29) + 1]
        ks += [rng.randrange(1 << 30) for _ in range(n_random)] + [rng.randrange(1 << 12) for _ in range(256)]
        return [(k,) for k in ks]
    arity, bound, pre = FIELD_OPS[op]
    top = bound(F)
    if op == "fe_canon":
        top = 3 * F.m
    if op == "fe_inv":
        n_random = min(n_random, 192)                       # 380 products each: one lane's time, not a wavefront's
    edges = [v for v in edge_values(F, rng) if v < top]
    if op == "fe_is_canonical":
        edges = edge_values(F, rng) + [MASK, MASK - 1]
    rnd = lambda n: random_values(F, rng, n, top if top < R else None)
    if arity == 1:
        cases = [(v,) for v in edges] + [(v,) for v in rnd(n_random)]
    elif arity == 2:
        cases = [(a, b) for a in edges for b in edges] + list(zip(rnd(n_random), rng.sample(rnd(n_random), n_random)))
    else:
        hi = sorted(v for v in edges if v >= F.m)
        cases = [(a, b, a, b) for a in edges for b in edges] + [(a, b, c, d) for a in hi[-6:] for b in hi[-6:] for c in hi[-3:] for d in hi[-3:]]
        cols = [rng.sample(rnd(n_random), n_random) for _ in range(4)]
        cases += list(zip(*cols))
        # operands in [m, 2m) throughout: the band where the scan most often ends above 2^255
        cases += [tuple(rng.randrange(F.m, 2 * F.m) for _ in range(4)) for _ in range(512)]
    if pre is not None:
        cases = [t for t in cases if pre(F, t)]
    return cases


NEG_LAZY_MULTIPLES = lambda F: [(k * F.m,) for k in range(4)]      # 3m - a is exact there too (only fe_canon's image is not 0)


# ---- crafted accumulator states for the lazy additions ---------------------------------------------------------------------
class LazyCase:
    """one lane: stored accumulator (any representatives), flags, the canonical point to add, and what the case is for"""
    def __init__(self, kind, acc, have, flip, b, on_curve, stored=None, addend=None):
        self.kind, self.acc, self.have, self.flip, self.b, self.on_curve = kind, tuple(acc), have, flip, tuple(b), on_curve
        self.stored, self.addend = stored, addend               # oracle points (on-curve cases)


def _reps(F, rng, acc, slack2):
    """move each coordinate to v, v + m or v + 2m, whichever of them (chosen at random) is inside the invariant"""
    out = []
    for v, k in zip(acc, slack2):
        c = [w for w in (v, v + F.m, v + 2 * F.m) if w < limit(F, k)]
        out.append(rng.choice(c))
    return tuple(out)


def _small_coord_state(F, rng, pt, which):
    """a state of `pt` whose X (which = 0) or ZZ (which = 2) Montgomery residue is tiny, so that v + 2m is inside the invariant"""
    m = F.m
    for t in range(1, 4096):
        zz = o.from_mont(t, m) * (pow(pt[0], -1, m) if which == 0 else 1) % m
        z = o.sqrt_mod(zz, m)
        if z:
            acc = list(xyzz_mont(F, pt, z))
            assert acc[which] == t
            return acc
    raise AssertionError("no square found")


def _same_x_states(F, S, want, lazy_add, rng):
    """stored accumulators of S whose P' against b = (x_S, .) is exactly `want` in {0, m, 2m}.  madd: P' = X - U2 with
    U2 = redc(x_b ZZ), so X = U2 + want (or U2 - m for want = m); want = 2m needs U2 < eps, found by choosing zz so that
    x_S zz = u / R for a tiny u and keeping the representative of ZZ for which redc returns u itself."""
    m = F.m
    bx = o.to_mont(S[0], m)
    if lazy_add:
        # P' = U1 - U2 (+ 2m): U1 = redc(X zz_b), U2 = redc(x_b ZZ); search z and representatives
        for _ in range(4096):
            z, zb = rng.randrange(1, m), rng.randrange(1, m)
            acc = list(xyzz_mont(F, S, z))
            b = xyzz_mont(F, S, zb)
            for dx in (0, m):
                for dz in (0, m):
                    a2 = [acc[0] + dx, acc[1], acc[2] + dz, acc[3]]
                    if fe_sub_lazy(F, fe_mul_lazy(F, a2[0], b[2]), fe_mul_lazy(F, b[0], a2[2])) == want:
                        return a2, zb
        raise AssertionError("unreachable P'")
    if want < 2 * m:
        z = rng.randrange(1, m)
        acc = list(xyzz_mont(F, S, z))
        acc[2] += rng.choice((0, m))
        U2 = fe_mul_lazy(F, bx, acc[2])
        acc[0] = U2 + want if U2 + want < limit(F, MADD_SLACK2[0]) else U2 - (2 * m - want)
        assert 0 <= acc[0] < limit(F, 2)
        return acc, None
    # U2 = redc(x_b ZZ) >= x_b ZZ / R, so U2 < eps needs a small product AND a small residue x_S zz R: a tiny Montgomery ZZ = t
    # (then U2 is the residue x_S t mod m itself) under a point with a tiny plain x (the caller passes one: small_x_point)
    assert S[0] < 1 << 32
    for t in range(1 + rng.randrange(64), 4096):
        z = o.sqrt_mod(o.from_mont(t, m), m)
        if not z:
            continue
        acc = list(xyzz_mont(F, S, z))
        U2 = fe_mul_lazy(F, bx, acc[2])
        assert acc[2] == t and U2 == S[0] * t and U2 < F.eps
        acc[0] = U2 + 2 * m
        return acc, None
    raise AssertionError("no square found")


def small_x_point(F, i):
    """the i-th point of the curve with a small plain x (no discrete logarithm known or needed)"""
    x = 0
    while True:
        x += 1
        y = o.sqrt_mod((x * x * x + o.CURVE_B) % F.m, F.m)
        if y:
            if i == 0:
                return (x, y)
            i -= 1


def lazy_cases(F, lazy_add, seed=3, n_general=96):
    """states for xyzz_madd_lazy (lazy_add False: b affine) or xyzz_add_lazy (True: b XYZZ, canonical), interleaved so every
    kind sits next to general additions in each wavefront.  Every emitted state passes the model's preconditions."""
    rng = random.Random((seed << 8) | F.fid | (16 if lazy_add else 0))
    m = F.m
    slack2 = ADD_SLACK2 if lazy_add else MADD_SLACK2
    pts = [mul_g(F, rng.randrange(2, 1 << 24)) for _ in range(24)]
    kinds = {}

    def addend(pt):
        """the operand for adding `pt` to the STORED accumulator, in the encoding the function takes"""
        return xyzz_mont(F, pt, rng.randrange(1, m)) if lazy_add else affine_mont(F, pt)

    def emit(kind, acc, have, flip, b, on, stored=None, add=None):
        kinds.setdefault(kind, []).append(LazyCase(kind, acc, have, flip, b, on, stored, add))

    for i in range(n_general):
        S, B = rng.choice(pts), rng.choice(pts)
        while B[0] == S[0]:
            B = rng.choice(pts)
        flip = i & 1
        acc = _reps(F, rng, xyzz_mont(F, S, rng.randrange(1, m) if i % 5 else 1), slack2)
        emit("general", acc, 1, flip, addend(B), True, S, B)
    for i in range(12):
        B = rng.choice(pts)
        junk = tuple(rng.randrange(lazy_top(F)) for _ in range(4))
        emit("first", junk, 0, i & 1, addend(B), True, None, B)
    for i in range(24):
        S, B = pts[i % 24], pts[(i + 7) % 24]
        acc = _small_coord_state(F, rng, S, (0, 2)[i & 1])
        w = (0, 2)[i & 1]
        acc[w] += (i // 2 % 3) * m                                     # v, v + m, v + 2m
        assert inside(F, acc, slack2)
        emit("small", acc, 1, (i >> 2) & 1, addend(B), True, S, B)
    for i in range(32):                                                 # coordinates at the top of their slack: off the curve
        B = rng.choice(pts)
        acc = tuple(limit(F, k) - 1 - (rng.randrange(1 << 64) if i >= 4 else i // 2) for k in slack2)
        if i % 4 == 3:                                                  # one coordinate at the top, the others anywhere
            j = rng.randrange(4)
            acc = tuple(v if jj == j else rng.randrange(limit(F, slack2[jj])) for jj, v in enumerate(acc))
        emit("top", acc, 1, i & 1, addend(B), False)
    wants = (0, m) if lazy_add else (0, m, 2 * m)
    for i in range(8 * len(wants)):
        want, flip, cancel = wants[i % len(wants)], (i // len(wants)) & 1, (i // (2 * len(wants))) & 1
        S = small_x_point(F, i) if want == 2 * m else pts[i % 24]
        acc, zb = _same_x_states(F, S, want, lazy_add, rng)
        B = o.pt_neg(S, m) if cancel else S
        b = xyzz_mont(F, B, zb) if lazy_add else affine_mont(F, B)
        emit(("cancel" if cancel else "double") + "_P%d" % (want // m), acc, 1, flip, b, True, S, B)
    # model preconditions hold for all of them (raises otherwise), and the tags are what they claim
    step = xyzz_add_lazy if lazy_add else xyzz_madd_lazy
    for k, lst in kinds.items():
        for c in lst:
            assert inside(F, c.acc, slack2) or not c.have
            _, _, _, Pn = step(F, c.acc, c.have, c.flip, c.b)
            if k.startswith(("double", "cancel")):
                assert Pn == int(k[-1]) * m, (k, Pn)
            elif c.have:
                assert Pn % m != 0
    # interleave: round-robin over the kinds
    order, lists = [], [list(v) for _, v in sorted(kinds.items())]
    while any(lists):
        for lst in lists:
            if lst:
                order.append(lst.pop())
    return order


def lazy_expected_point(F, c):
    """the group element the resolved output must be (on-curve cases): sigma_in (stored + b), or b itself on the first branch;
    `addend` was passed to the stored accumulator as is"""
    m = F.m
    if not c.have:
        return c.addend
    s = o.pt_add(c.stored, c.addend, m)
    return o.pt_neg(s, m) if c.flip else s


def slack_in_eps(F, v):
    return Fraction(v - 2 * F.m, F.eps)


# ---- group-law cases: rows of words for the runner, with the oracle point each output must be --------------------------------
def _pool(F, rng, n=16):
    return [mul_g(F, rng.randrange(2, 1 << 24)) for _ in range(n)]


def _pair_kinds(F, rng, pts, i):
    """(A, B, kind) cycling through general / P + P / P + (-P) / identity left / identity right / both identity"""
    A, B = pts[i % len(pts)], pts[(3 * i + 1) % len(pts)]
    kind = ("general", "double", "opposite", "id_left", "id_right", "general", "double", "opposite", "id_both", "general")[i % 10]
    if kind == "general" and A[0] == B[0]:
        B = o.pt_add(B, o.generator(F.curve), F.m)
    if kind == "double":
        B = A
    if kind == "opposite":
        B = o.pt_neg(A, F.m)
    if kind in ("id_left", "id_both"):
        A = None
    if kind in ("id_right", "id_both"):
        B = None
    return A, B, kind


def _z(F, rng, i):
    return 1 if i % 7 == 3 else rng.randrange(1, F.m)          # mostly non-trivial zz, sometimes a fresh accumulator


def group_cases(F, op, seed=5, n=101):
    """-> (rows, expected): one full wavefront and a partial one; expected[i] is an oracle point (None = identity)"""
    rng = random.Random((seed << 8) | F.fid)
    m = F.m
    pts = _pool(F, rng)
    rows, exp = [], []
    for i in range(n):
        A, B, _ = _pair_kinds(F, rng, pts, i)
        if op in ("xyzz_madd", "xyzz_madd_inl"):
            rows.append(xyzz_mont(F, A, _z(F, rng, i)) + affine_mont(F, B)); exp.append(o.pt_add(A, B, m))
        elif op == "xyzz_add":
            rows.append(xyzz_mont(F, A, _z(F, rng, i)) + xyzz_mont(F, B, _z(F, rng, i + 1))); exp.append(o.pt_add(A, B, m))
        elif op == "xyzz_dbl":
            rows.append(xyzz_mont(F, A, _z(F, rng, i))); exp.append(o.pt_add(A, A, m))
        elif op == "xyzz_dbl_affine":
            A = A or pts[i % len(pts)]
            rows.append(affine_mont(F, A)); exp.append(o.pt_add(A, A, m))
        elif op in ("xyzz_to_jac", "xyzz_to_affine"):
            rows.append(xyzz_mont(F, A, _z(F, rng, i))); exp.append(A)
        elif op == "jac_to_xyzz":
            z = _z(F, rng, i)
            rows.append((0, 0, 0) if A is None else tuple(o.to_mont(v, m) for v in (A[0] * z * z, A[1] * z * z * z, z)))
            exp.append(A)
        elif op == "xyzz_mul_u64":
            A = A or pts[i % len(pts)]
            k = (0, 1, 2, 3, (1 << 64) - 1, 1 << 63, (1 << 32) - 1, 1 << 32)[i] if i < 8 else rng.randrange(1 << 64)
            if i >= 40:
                k >>= 40                                              # the Python reference pays an inversion per bit
            rows.append(affine_mont(F, A) + (k,)); exp.append(o.pt_mul(k, A, m))
        else:
            raise KeyError(op)
    return rows, exp


def quad_cases(F, op, seed=7, n=55):
    """QPoint ops: 16 quads of a wavefront hold different kinds side by side (the kinds cycle with period 10)"""
    rng = random.Random((seed << 8) | F.fid)
    m = F.m
    pts = _pool(F, rng)
    rows, exp = [], []
    for i in range(n):
        A, B, _ = _pair_kinds(F, rng, pts, i)
        if op == "qpoint_add":
            rows.append(xyzz_mont(F, A, _z(F, rng, i)) + xyzz_mont(F, B, _z(F, rng, i + 1))); exp.append(o.pt_add(A, B, m))
        elif op == "qpoint_dbl":
            rows.append(xyzz_mont(F, A, _z(F, rng, i))); exp.append(o.pt_add(A, A, m))
        elif op == "qpoint_neg":
            rows.append(xyzz_mont(F, A, _z(F, rng, i))); exp.append(o.pt_neg(A, m))
        else:
            raise KeyError(op)
    return rows, exp


def load_lazy_cases(F, seed=9, n=55):
    """qpoint_load_lazy -> qpoint_store: lazy representatives of every coordinate (v, v + m, v + 2m below 2m + 9 eps; a flushed
    y may be fe_neg_lazy's 3m - y), the all-zero identity and zz = m / 2m.  -> (rows, expected rows, expected inf)"""
    rng = random.Random((seed << 8) | F.fid)
    m = F.m
    pts = _pool(F, rng)
    rows, out, inf = [], [], []
    for i in range(n):
        can = list(xyzz_mont(F, pts[i % len(pts)], _z(F, rng, i)))
        row = [rng.choice([w for w in (v, v + m, v + 2 * m) if w < lazy_top(F)]) for v in can]
        if i % 4 == 1:
            row[1] = 3 * m - ((m - can[1]) + rng.choice((0, m)))      # what xyzz_lazy_resolve stores under a pending sign
        if i % 11 == 5:
            row = [0, 0, 0, 0]
        if i % 11 == 7:
            row[2] = m * (1 + (i & 1))                                   # zz = 0 (mod m) in a lazy representation
        c = [fe_canon(F, v) for v in row]
        rows.append(tuple(row)); inf.append(int(c[2] == 0)); out.append((0, 0, 0, 0) if c[2] == 0 else tuple(c))
    return rows, out, inf


WAVE_SUM_SCALARS = (
    [1] * 16,                                                           # every butterfly step doubles
    [1] * 8 + [-1] * 8,                                                 # the first step cancels everywhere, the rest add identities
    [1, 2, 3, 4, 5, 6, 7, 8, 1, 2, -3, -4, 9, 10, 11, 12],              # step 1: doubles, cancels, general; step 3: 20 + 20 doubles
    [7] * 4 + [-7] * 4 + [7] * 4 + [-7] * 4,                            # step 1 doubles (quads i, i + 8), step 2 cancels (i, i + 4)
    [0, 5, 0, 0, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 11],                  # mostly identities
    None,                                                               # random
)


def wave_sum_cases(F, seed=11):
    """16 points per wavefront (quad i pairs with i ^ 8, ^ 4, ^ 2, ^ 1).  -> (rows, expected point per case)"""
    rng = random.Random((seed << 8) | F.fid)
    base = mul_g(F, rng.randrange(2, 1 << 24))
    rows, exp = [], []
    for sc in WAVE_SUM_SCALARS:
        sc = sc or [rng.randrange(-1000, 1000) for _ in range(16)]
        for k in sc:
            rows.append(xyzz_mont(F, o.pt_mul(k, base, F.m) if k else None, rng.randrange(1, F.m)))
        exp += [o.pt_mul(sum(sc), base, F.m) if sum(sc) else None] * 16
    return rows, exp


# ---- the runner's job files (tools/ubench/prim_check.hip) ------------------------------------------------------------------
import os
import struct
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIM_CHECK = os.path.join(ROOT, "tools", "ubench", "prim_check")
# name -> (op id, words in, words out, runs with --host)
OPS = {
    "fe_mul_lazy": (1, 2, 1, 1), "fe_sqr_lazy": (2, 1, 1, 1), "fe_mul_inl": (3, 2, 1, 1), "fe_sqr_inl": (4, 1, 1, 1),
    "fe_mul2_lazy": (5, 4, 1, 1), "fe_sub_lazy": (6, 2, 1, 1), "fe_neg_lazy": (7, 1, 1, 1), "fe_neg_nz": (8, 1, 1, 1),
    "fe_canon": (9, 1, 1, 1), "fe_add": (10, 2, 1, 1), "fe_sub": (11, 2, 1, 1), "fe_neg": (12, 1, 1, 1), "fe_dbl": (13, 1, 1, 1),
    "fe_from_small": (14, 1, 1, 1), "fe_from_mont": (15, 1, 1, 1), "fe_to_mont": (16, 1, 1, 1), "fe_inv": (17, 1, 1, 1),
    "fe_is_canonical": (18, 1, 1, 1), "fe_mul": (19, 2, 1, 1),
    "xyzz_madd_lazy": (20, 8, 10, 1), "xyzz_add_lazy": (21, 10, 10, 0),
    "xyzz_madd": (22, 6, 4, 1), "xyzz_madd_inl": (23, 6, 4, 1), "xyzz_add": (24, 8, 4, 1), "xyzz_dbl": (25, 4, 4, 1),
    "xyzz_dbl_affine": (26, 2, 4, 1), "xyzz_to_jac": (27, 4, 3, 1), "jac_to_xyzz": (28, 3, 4, 1), "xyzz_to_affine": (29, 4, 2, 1),
    "xyzz_mul_u64": (30, 3, 4, 1),
    "qpoint_add": (40, 8, 5, 0), "qpoint_dbl": (41, 4, 5, 0), "qpoint_neg": (42, 4, 5, 0), "qpoint_load_lazy": (43, 4, 5, 0),
    "qpoint_wave_sum": (44, 4, 5, 0),
}
GROUP_OPS = ("xyzz_madd", "xyzz_madd_inl", "xyzz_add", "xyzz_dbl", "xyzz_dbl_affine", "xyzz_to_jac", "jac_to_xyzz", "xyzz_to_affine",
             "xyzz_mul_u64")


def run_jobs(jobs, host=False, timeout=120):
    """jobs: [(field, op name, rows of integers)] -> [rows of integers], through ONE child process"""
    assert os.path.exists(PRIM_CHECK), "tools/ubench/prim_check is not built: make -C vdf_amd/csrc"
    blob = [b"PRIMJOB1", struct.pack("<I", len(jobs))]
    for F, op, rows in jobs:
        oid, nin, _, host_ok = OPS[op]
        assert host_ok or not host, op
        assert all(len(r) == nin for r in rows), op
        blob.append(struct.pack("<4I", F.fid, oid, len(rows), nin))
        blob.append(b"".join(int(v).to_bytes(32, "little") for r in rows for v in r))
    with tempfile.TemporaryDirectory() as d:
        jf, rf = os.path.join(d, "jobs.bin"), os.path.join(d, "results.bin")
        with open(jf, "wb") as f:
            f.write(b"".join(blob))
        r = subprocess.run([PRIM_CHECK] + (["--host"] if host else []) + [jf, rf], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, "prim_check exit %d: %s%s" % (r.returncode, r.stdout, r.stderr)
        with open(rf, "rb") as f:
            data = f.read()
    assert data[:8] == b"PRIMOUT1" and struct.unpack_from("<I", data, 8)[0] == len(jobs)
    pos, res = 12, []
    for F, op, rows in jobs:
        oid, _, nout, _ = OPS[op]
        assert struct.unpack_from("<4I", data, pos) == (F.fid, oid, len(rows), nout)
        pos += 16
        out = []
        for _ in rows:
            out.append(tuple(int.from_bytes(data[pos + 32 * k: pos + 32 * k + 32], "little") for k in range(nout)))
            pos += 32 * nout
        res.append(out)
    assert pos == len(data)
    return res


def check_group(F, op, rows, exp, got):
    """outputs of a canonical group-law function as group elements (and canonical coordinates) against the oracle"""
    m = F.m
    for i, (g, e) in enumerate(zip(got, exp)):
        assert all(v < m for v in g), (op, i)
        if op == "xyzz_to_affine":
            assert g == affine_mont(F, e), (op, i)
            continue
        pt = jac_point(F, g) if op == "xyzz_to_jac" else xyzz_point(F, g)
        assert pt == e, "%s %s case %d" % (F, op, i)
        if e is not None:
            assert o.on_curve(pt, F.curve)


def lazy_rows(cases):
    return [c.acc + (c.have, c.flip) + c.b for c in cases]


def lazy_model_row(F, lazy_add, c):
    """the ten output words of the runner for one lazy addition"""
    acc, have, flip, _ = (xyzz_add_lazy if lazy_add else xyzz_madd_lazy)(F, c.acc, c.have, c.flip, c.b)
    return tuple(acc) + (have, flip) + xyzz_lazy_resolve(F, acc, have, flip)
