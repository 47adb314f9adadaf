"""Forward bodies (include/vdf_nova.h vdf_nova_forward_body_record, vdf_cs_pow; include/vdf_hip.h vdf_round_tape_forward_walk)
for the CPU and the GPU tests: the two test bodies, a big-integer model of a forward walk and of the layout it writes
(oracle/pasta.py integers: the reference of the host evaluator and of the kernel), and the shared cases.

M  the MinRoot forward round (src/minroot.rs:329-335) as a forward body: n_adv = 2 (x, y), no inv: next.x = (x + y)^e with
   e = 5^-1 mod (m - 1), computed here; next.y = x + j.  The chain's counter is j: a walk whose state has counter i runs under
   j_base = i.
E  a body of three columns (a, b, c) that uses every arithmetic op and six powers:
     d = a + b - k, e = d c, g = 7 e^2,
     h = g + 11 + j + g^0 + d^1 + c^2 + a^(2^255) + b^(2^255 - 1) + e^(m - 2);      next = (h, a, h)
   -- ADD, SUB, MUL, a squaring, SCALE, CONST, INV, J and POW; column 1 is an input passed through (from column 0: an OUT of a
   column a later round reads), and one handle feeds columns 0 and 2.  e^(m - 2) is the inverse of e (0 for e = 0)."""
import numpy as np

from oracle import pasta as o
from rounds_spec import MOD, fe, mont_rows  # noqa: F401  (mont_rows: for the tests that import this module)
from walks_spec import GUARD, expected_bytes, guarded, start_entries, tape_ints  # noqa: F401
from vdf_amd.nova import WalkBody

TAPE_POW = 9


def root_exponent(field):
    m = MOD[field]
    return pow(5, -1, m - 1)


def minroot_forward_body(field):
    e = root_exponent(field)

    def b(cs, j, inv, cur):
        return [cs.pow(cs.add(cur[0], cur[1]), e), cs.add(cur[0], j)]
    return WalkBody(0, 2, b)


def minroot_forward_ints(cur, j, inv, m):
    x, y = cur
    return [pow((x + y) % m, pow(5, -1, m - 1), m), (x + j) % m]


def every_op_exponents(m):
    return [0, 1, 2, 2**255, 2**255 - 1, m - 2]


def every_op_forward_body(field):
    m = MOD[field]
    E = every_op_exponents(m)

    def b(cs, j, inv, cur):
        d = cs.sub(cs.add(cur[0], cur[1]), inv[0])
        e = cs.mul(d, cur[2])
        g = cs.scale(cs.mul(e, e), fe(7, m))
        h = cs.add(cs.add(g, cs.const(fe(11, m))), j)
        for base, ex in zip((g, d, cur[2], cur[0], cur[1], e), E):
            h = cs.add(h, cs.pow(base, ex))
        return [h, cur[0], h]
    return WalkBody(1, 3, b)


def every_op_forward_ints(cur, j, inv, m):
    a, b, c = cur
    d = (a + b - inv[0]) % m
    e = d * c % m
    g = 7 * e * e % m
    h = g + 11 + j
    for base, ex in zip((g, d, c, a, b, e), every_op_exponents(m)):
        h += pow(base, ex, m)
    assert e * pow(e, m - 2, m) % m == (1 if e else 0)           # the last power is the inversion
    h %= m
    return [h, a, h]


def pow_products(e):
    """what the header counts for a POW of exponent e"""
    return max(1, e.bit_length() - 1 + bin(e).count("1") - 1)


def model_forward(fn, m, na, inv, entries, n, rounds, checkpoints=None, every=0, cp_stride=0, trace=None, walk_stride=0, base=0,
                  j_base=0, j_walk_step=0):
    """The contract of vdf_round_tape_forward_walk over Python ints: entries (flat, n x na), checkpoints and trace (flat lists, or
    None) in place."""
    for w in range(n):
        cur = entries[w * na:(w + 1) * na]
        for r in range(rounds):
            j = (j_base + w * j_walk_step + base + r) % 2**64
            cur = fn(cur, j % m, inv, m)
            g = base + r + 1
            if trace is not None:
                trace[(w * walk_stride + g) * na:(w * walk_stride + g + 1) * na] = cur
            if checkpoints is not None and g % every == 0:
                k = w * cp_stride + g // every
                checkpoints[k * na:(k + 1) * na] = cur
        entries[w * na:(w + 1) * na] = cur


# the layout case of both test files: n = 6 walks that have `base` = 3 rounds behind them and run 5 more; a trace run every 11
# entries (9 would do), checkpoint runs `cp_stride` apart; FRONT guard entries in front of both arrays; j runs on by 1000 per walk
# from just below 2^64
LAYOUT = dict(n=6, rounds=5, walk_stride=11, base=3, j_base=2**64 - 5, j_walk_step=1000)
LAYOUT_FRONT = 2
LAYOUT_TRACE = LAYOUT_FRONT + 6 * 11 + 1
CP_STRIDE = {1: 10, 2: 6, 5: 3}                       # checkpoints 4 .. 8, 2 .. 4 and 1 of a walk; one entry or more between the runs


def layout_cp_entries(every):
    return LAYOUT_FRONT + 6 * CP_STRIDE[every] + 1


def layout_expected(field, every, rng_seed=5):
    """(starting entries ints, inv ints, trace ints and checkpoint ints with None where nothing may be written (front guards
    included), landings)"""
    m = MOD[field]
    rng = np.random.default_rng(rng_seed + field)
    start = start_entries(LAYOUT["n"], 3, m, rng)
    inv = [0x1234567 % m]
    trace = [None] * (3 * (LAYOUT_TRACE - LAYOUT_FRONT))
    cps = [None] * (3 * (layout_cp_entries(every) - LAYOUT_FRONT))
    land = list(start)
    model_forward(every_op_forward_ints, m, 3, inv, land, checkpoints=cps, every=every, cp_stride=CP_STRIDE[every], trace=trace, **LAYOUT)
    front = [None] * (3 * LAYOUT_FRONT)
    return start, inv, front + trace, front + cps, land
