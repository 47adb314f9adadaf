"""Shared by the tests of the periodic rows (include/vdf_hip.h vdf_periodic_rows): a test circuit whose rows are NOT periodic,
the operands of a cross term with the edge values in place, and the big-integer sparse product that is the reference of the
host evaluator (oracle/pasta.py integers), which in turn is the reference of the kernel.

Acc  a carry that accumulates: arity 2, z = (a, k); carry (a), inv = (k), n_adv = 2 with columns (a_j, u_j):
       u = alloc_from(cur[1]); p = a * u (a variable and its constraint); a' = a + u.
     The linear combination of the carry is a_0 + u_0 + .. + u_(j-1): row j has j + 1 terms, so no repetition repeats the one
     before it.  Advice: u free, a_(j+1) = a_j + u_j.  z_out = (a_t, k)."""
import functools

import numpy as np

from oracle import pasta as o
from rounds_spec import F, G, MOD, _Rounds
from util import ints, limbs
from vdf_amd.hip import TERM_ABS, TERM_SEG
from vdf_amd.nova import RoundBody, shape_export_custom, shape_periodic_custom

NUM_IO = 2


class Acc(_Rounds):
    arity, n_adv, n_vars = 2, 2, 2

    def body(self):
        def b(cs, j, inv, carry, cur, nxt):
            u = cs.alloc_from(cur[1])
            cs.mul(carry[0], u)
            return [cs.add(carry[0], u)]
        return RoundBody(1, 1, 2, b)

    def synthesize(self, cs, z):
        a, k = z
        (a,) = cs.repeat(self.body(), self.t, [k], [a], self.advice if cs.is_witness else None)
        return [a, k]

    @staticmethod
    def advice_for(a0, t, m, rng):
        adv, a = [], a0 % m
        for _ in range(t + 1):
            u = int(rng.integers(1, 2**62)) ** 4 % m
            adv += [a, u]
            a = (a + u) % m
        return adv


CIRCUITS = {"F": F, "G": G, "Acc": Acc}


@functools.lru_cache(maxsize=None)
def described(name, t, field):
    """(triples of the primary shape, description or None, info) of circuit `name` at t over `field`, made once"""
    c = CIRCUITS[name](t, "repeat", field)
    mats = shape_export_custom(c, field)
    pr, info = shape_periodic_custom(c, field)
    return mats, pr, info


def operands(field, info, pr, seed):
    """z2, Az1, Bz1, Cz1 (uint64[n, 4], Montgomery, every element canonical), u1 (uint64[1, 4]): arbitrary values, with 0, 1 and
    p - 1 among the variables the periodic rows read, and a `one` that is not 1"""
    m = MOD[field]
    rng = np.random.default_rng(seed)

    def rand(n):
        a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        return a
    z2 = rand(info["num_cols"])
    first = info["seg_begin"] + pr.lead * pr.c.n_vars
    special = limbs([o.to_mont(v, m) for v in (0, 1, m - 1)])
    for k in range(6):                                     # among the variables of the first two periodic repetitions
        z2[first + k] = special[k % 3]
    z2[info["num_cols"] - 1 - NUM_IO] = limbs([o.to_mont(0x1234567, m)])[0]      # the constant's column
    return z2, rand(info["num_cons"]), rand(info["num_cons"]), rand(info["num_cons"]), rand(1)


def sparse_reference(field, mats, row_begin, row_count, z2, az1, bz1, cz1, u1):
    """Az2, Bz2, Cz2, T (uint64[row_count, 4], Montgomery) of the rows [row_begin, row_begin + row_count) by big integers over the
    triples: the sparse product, then T = Az1 o Bz2 + Az2 o Bz1 - u1 Cz2 - Cz1"""
    m = MOD[field]
    fm = lambda arr: [o.from_mont(v, m) for v in ints(arr)]
    abc = []
    for rows, cols, vals in mats:
        sel = np.nonzero((rows >= row_begin) & (rows < row_begin + row_count))[0]
        acc = [0] * row_count
        zs, vs = fm(z2[cols[sel]]), fm(vals[sel])
        for e, r in enumerate(rows[sel]):
            acc[int(r) - row_begin] += vs[e] * zs[e]
        abc.append([v % m for v in acc])
    sl = slice(row_begin, row_begin + row_count)
    a1, b1, c1, (u,) = fm(az1[sl]), fm(bz1[sl]), fm(cz1[sl]), fm(u1)
    T = [(a1[i] * abc[1][i] + abc[0][i] * b1[i] - u * abc[2][i] - c1[i]) % m for i in range(row_count)]
    return [limbs([o.to_mont(v, m) for v in vec]) for vec in abc + [T]]


GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)


def guarded(n):
    """four output vectors of n elements filled with a pattern no field element has"""
    return [np.full((n, 4), GUARD, dtype="<u8") for _ in range(4)]


def refusal_cases(pr, info, t):
    """(name, mutate(pr) -> undo, call overrides): each makes the description or the call malformed in one way"""
    term = pr.terms
    seg0 = next(i for i in range(pr.c.n_terms) if term[i].kind == TERM_SEG)
    back = min(range(pr.c.n_terms), key=lambda i: term[i].col - (1 << 32) if term[i].kind == TERM_SEG and term[i].col >> 31 else 0)
    abs0 = next(i for i in range(pr.c.n_terms) if term[i].kind == TERM_ABS)

    def setter(i, name, value):
        def f():
            old = getattr(term[i], name)
            setattr(term[i], name, value)
            return lambda: setattr(term[i], name, old)
        return f
    nothing = lambda: (lambda: None)
    return [
        ("a bad kind", setter(seg0, "kind", 2), {}),
        ("a bad constant index", setter(seg0, "c0", pr.c.n_consts), {}),
        ("a bad slope index", setter(abs0, "c1", pr.c.n_consts), {}),
        ("a fixed column at num_cols", setter(abs0, "col", info["num_cols"]), {}),
        ("a reachable column at num_cols", setter(seg0, "col", info["num_cols"] - info["seg_begin"] - (t - 1) * pr.c.n_vars), {}),
        ("a reach below column 0", setter(back, "col", (1 << 32) - (info["seg_begin"] + pr.lead * pr.c.n_vars + 1)), {}),
        ("a row range beyond num_cons", nothing, {"row_begin": info["num_cons"] - pr.row_count + 1}),
        ("a first repetition before the pattern's", nothing, {"j_first": pr.lead - 1}),
        ("more columns than the vectors have", nothing, {"num_cols": info["seg_begin"] + t * pr.c.n_vars - 1}),
    ]
