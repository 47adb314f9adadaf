"""Walk bodies (include/vdf_nova.h vdf_walk_body; include/vdf_hip.h vdf_round_tape_walk) for the CPU and the GPU tests: the two
test bodies, a big-integer model of a walk and of the layout it writes (oracle/pasta.py integers: the reference of the host
evaluator and of the kernel), and the shared cases.

M  the MinRoot inverse round (src/minroot.rs:338-344) as a walk body: n_adv = 2 (x, y), inv = (inv0), the chain's starting
   counter: cur.x = next.y - (inv0 + j), cur.y = next.x^5 - cur.x.  Entry k of a chain is the state whose counter is inv0 + k.
E  a body of three columns (a, b, c) that uses every op: h = 7 ((a + b - k) c)^2 + 11 + j; cur = (h, a, h) -- ADD, SUB, MUL, a
   squaring, SCALE, CONST, INV and J; column 1 is an input passed through (from column 0: an OUT of a column a later round reads),
   and one handle feeds columns 0 and 2."""
import numpy as np

from oracle import pasta as o
from rounds_spec import MOD, fe, mont_rows
from util import ints
from vdf_amd.nova import WalkBody

GUARD = 2**64 - 1          # every word of an element nothing may write


def minroot_body(field):
    def b(cs, j, inv, nxt):
        cx = cs.sub(nxt[1], cs.add(inv[0], j))
        x2 = cs.mul(nxt[0], nxt[0])
        x5 = cs.mul(cs.mul(x2, x2), nxt[0])
        return [cx, cs.sub(x5, cx)]
    return WalkBody(1, 2, b)


def every_op_body(field):
    m = MOD[field]

    def b(cs, j, inv, nxt):
        d = cs.sub(cs.add(nxt[0], nxt[1]), inv[0])
        e = cs.mul(d, nxt[2])
        g = cs.scale(cs.mul(e, e), fe(7, m))
        h = cs.add(cs.add(g, cs.const(fe(11, m))), j)
        return [h, nxt[0], h]
    return WalkBody(1, 3, b)


def every_op_ints(nxt, j, inv, m):
    a, b, c = nxt
    h = (7 * pow((a + b - inv[0]) * c, 2, m) + 11 + j) % m
    return [h, a, h]


def minroot_ints(nxt, j, inv, m):
    x, y = nxt
    cx = (y - inv[0] - j) % m
    return [cx, (pow(x, 5, m) - cx) % m]


def model_walk(fn, m, na, inv, entries, n, rounds, trace=None, walk_stride=0, top=0, group=0, group_stride=0, j_base=0, j_group_step=0,
               heads=False):
    """The contract of vdf_round_tape_walk over Python ints: entries (flat, n x na) and trace (flat list, or None) in place."""
    if group == 0:
        group, group_stride = n, 0
    for w in range(n):
        g, first = w // group, (w % group) * walk_stride + top
        cur = entries[w * na:(w + 1) * na]
        for r in range(rounds):
            k = first - r
            if trace is not None:
                assert k >= 0
                trace[(g * group_stride + k) * na:(g * group_stride + k + 1) * na] = cur
            j = (j_base + g * j_group_step + k - 1) % 2**64
            cur = fn(cur, j % m, inv, m)
        entries[w * na:(w + 1) * na] = cur
        if trace is not None and heads and w % group == 0:
            k = first - rounds
            assert k >= 0
            trace[(g * group_stride + k) * na:(g * group_stride + k + 1) * na] = cur


def guarded(n_elems):
    return np.full((n_elems, 4), GUARD, dtype="<u8")


def expected_bytes(trace_ints, m):
    """a flat list of ints (None = untouched guard) -> the bytes of the uint64[., 4] array it must equal"""
    return b"".join(b"\xff" * 32 if v is None else int(o.to_mont(v, m)).to_bytes(32, "little") for v in trace_ints)


def start_entries(n, na, m, rng, special=(0, 1, -1)):
    """n x na starting values, 0, 1 and m - 1 among them"""
    vals = [int(rng.integers(0, 2**62)) ** 5 % m for _ in range(n * na)]
    for k, s in enumerate(special):
        vals[(3 * k + 1) % len(vals)] = s % m
    return vals


# the layout case of both test files: n = 6 walks in 3 groups of 2, walks of 5 rounds 5 entries apart, a group every 14 entries
# (11 would do), 3 guard entries in front; j runs on by 1000 per group
LAYOUT = dict(n=6, rounds=5, walk_stride=5, top=5, group=2, group_stride=14, j_base=77, j_group_step=1000)
LAYOUT_FRONT, LAYOUT_ENTRIES = 3, 3 + 3 * 14


def layout_expected(field, heads, rng_seed=5):
    """(starting entries ints, inv ints, trace ints with None where nothing may be written (front guard included), landings)"""
    m = MOD[field]
    rng = np.random.default_rng(rng_seed + field)
    start = start_entries(LAYOUT["n"], 3, m, rng)
    inv = [0x1234567 % m]
    trace = [None] * (3 * (LAYOUT_ENTRIES - LAYOUT_FRONT))
    land = list(start)
    model_walk(every_op_ints, m, 3, inv, land, trace=trace, heads=heads, **LAYOUT)
    return start, inv, [None] * (3 * LAYOUT_FRONT) + trace, land


def tape_ints(arr, m):
    return [o.from_mont(v, m) for v in ints(arr)]
