"""VDF_TAPE_TAB (include/vdf_hip.h) and vdf_cs_tab (include/vdf_nova.h) as big integers: the row rule, bodies of all three kinds
that use every op together with a table, models of the three calls that hand a round the RAW 64-bit counter (the models of
walks_spec / forward_tape_spec reduce it modulo the field first, and a row needs it whole), and the tabbed MinRoot round.

THE RULE.  slot = table[(J mod rows) * cols + a], J the 64-bit value VDF_TAPE_J has in that round: (j_base + ...) mod 2^64 first,
mod rows second.  The two do not commute for a `rows` that is no power of two, which is what the wrap cases pin.

R   a round body of three advice columns (a, u, w), inv (k), carry (a), table columns c0 and c1:
      u = alloc_from(cur[1]); w = alloc_from(3 (next[2] - cur[2])); p = u w; s = p - 7 a + (j + 11) + tab[c0]; q = s s; r = q k;
      e = q tab[c1], and q tab[c1] = e enforced once more; a' = r + u + e
    -- the table in a linear combination, as an operand of a product, in an enforce and in carry_out.  Variables u, w, p, q, r, e.
W   a descending walk body of three columns (a, b, c): h = 7 ((a + b - k) c)^2 + 11 + j + tab[c0] + tab[c1] c; cur = (h, a, h).
FW  a forward body of three columns: d = a + b - k, e = d c, g = 7 e^2,
      h = g + 11 + j + tab[c0] + d^5 (POW) + c^5 (POWC, when asked for) + tab[c1] a;  next = (h, a, h).
TM  MinRoot's round with a table in the place of the counter i (examples/prove_tabbed_chain.c): an entry is (x, y),
      forward x' = (x + y + c0[j])^(1/5), y' = x + c1[j];  walk x = y' - c1[j], y = x'^5 - x - c0[j];
      round xn = alloc_from(next[0]), t1 = xn^2, t2 = t1^2, t2 xn = x + y + c0[j] enforced, yn = x + c1[j].
    With c0 absent and c1[r] = i0 + r over rows >= the rounds walked it IS MinRoot from counter i0."""
import numpy as np

from oracle import pasta as o
from rounds_spec import MOD, fe, mont_rows
from util import limbs
from vdf_amd.nova import RoundBody, StepCircuit, WalkBody, FIELD_FQ

TAPE_TAB = 11
MAX_TAB_ROWS, MAX_TAB_COLS = 4096, 8
CHAIN5 = [(0, 2, 0, 0xFF)]             # x -> x^5: from T[0], two squarings, times T[0]


def tab_row(J, rows):
    return (J % 2**64) % rows


def table_ints(rows, cols, m, seed=1):
    """rows x cols values, 0 and m - 1 among them (entry 0 and the last one, and 1 where there is room)"""
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    vals = [int(rng.integers(0, 2**62)) ** 5 % m for _ in range(rows * cols)]
    vals[0] = 0
    vals[-1] = m - 1
    if len(vals) > 2:
        vals[len(vals) // 2] = 1
    return vals


def table_array(vals, rows, cols, m):
    """flat ints -> the uint64[rows, cols, 4] Montgomery array ConstraintSystem.tab and RoundTape.set_table take"""
    return np.ascontiguousarray(limbs([o.to_mont(v % m, m) for v in vals]).reshape(rows, cols, 4))


# ---- R, W, FW ------------------------------------------------------------------------------------------------------------------
def round_body(field, table, c0, c1):
    m = MOD[field]

    def b(cs, j, inv, carry, cur, nxt):
        u = cs.alloc_from(cur[1])
        w = cs.alloc_from(cs.scale(cs.sub(nxt[2], cur[2]), fe(3, m)))
        p = cs.mul(u, w)
        s = cs.sub(p, cs.scale(carry[0], fe(7, m)))
        s = cs.add(cs.add(s, cs.add(j, cs.const(fe(11, m)))), cs.tab(table, c0))
        q = cs.mul(s, s)
        r = cs.mul(q, inv[0])
        k1 = cs.tab(table, c1)
        e = cs.mul(q, k1)
        cs.enforce(q, k1, e)
        return [cs.add(cs.add(r, u), e)]
    return RoundBody(1, 1, 3, b)


def round_vars(adv, t, inv, m, tab, rows, cols, c0, c1):
    """the 6 t variables of R from the advice (flat ints, (t + 1) x 3)"""
    out = []
    for j in range(t):
        a, u = adv[3 * j], adv[3 * j + 1]
        w = 3 * (adv[3 * (j + 1) + 2] - adv[3 * j + 2]) % m
        row = tab_row(j, rows)
        p = u * w % m
        s = (p - 7 * a + j + 11 + tab[row * cols + c0]) % m
        q = s * s % m
        out += [u, w, p, q, q * inv[0] % m, q * tab[row * cols + c1] % m]
    return out


def round_advice(a0, k, t, m, rng, tab, rows, cols, c0, c1):
    """consistent advice of R: free u, w (0, 1 and m - 1 among them), a by the recurrence"""
    free = [0, 1, m - 1] + [int(rng.integers(0, 2**62)) ** 4 % m for _ in range(2 * (t + 1))]
    us, ws = free[:t + 1], free[t + 1:2 * (t + 1)]
    adv, a = [], a0 % m
    for j in range(t + 1):
        adv += [a, us[j], ws[j]]
        if j < t:
            row = tab_row(j, rows)
            w = 3 * (ws[j + 1] - ws[j]) % m
            s = (us[j] * w - 7 * a + j + 11 + tab[row * cols + c0]) % m
            q = s * s % m
            a = (q * k + us[j] + q * tab[row * cols + c1]) % m
    return adv


def walk_body(field, table, c0, c1):
    m = MOD[field]

    def b(cs, j, inv, nxt):
        d = cs.sub(cs.add(nxt[0], nxt[1]), inv[0])
        e = cs.mul(d, nxt[2])
        g = cs.scale(cs.mul(e, e), fe(7, m))
        h = cs.add(cs.add(g, cs.const(fe(11, m))), j)
        h = cs.add(cs.add(h, cs.tab(table, c0)), cs.mul(cs.tab(table, c1), nxt[2]))
        return [h, nxt[0], h]
    return WalkBody(1, 3, b)


def walk_ints(nxt, J, inv, m, tab, rows, cols, c0, c1):
    a, b, c = nxt
    row = tab_row(J, rows)
    h = (7 * pow((a + b - inv[0]) * c, 2, m) + 11 + J + tab[row * cols + c0] + tab[row * cols + c1] * c) % m
    return [h, a, h]


def forward_body(field, table, c0, c1, chain=False):
    m = MOD[field]

    def b(cs, j, inv, cur):
        d = cs.sub(cs.add(cur[0], cur[1]), inv[0])
        e = cs.mul(d, cur[2])
        g = cs.scale(cs.mul(e, e), fe(7, m))
        h = cs.add(cs.add(g, cs.const(fe(11, m))), j)
        h = cs.add(cs.add(h, cs.tab(table, c0)), cs.pow(d, 5))
        if chain:
            h = cs.add(h, cs.pow_chain(cur[2], CHAIN5))
        h = cs.add(h, cs.mul(cs.tab(table, c1), cur[0]))
        return [h, cur[0], h]
    return WalkBody(1, 3, b)


def forward_ints(cur, J, inv, m, tab, rows, cols, c0, c1, chain=False):
    a, b, c = cur
    row = tab_row(J, rows)
    d = (a + b - inv[0]) % m
    e = d * c % m
    h = 7 * e * e + 11 + J + tab[row * cols + c0] + pow(d, 5, m) + (pow(c, 5, m) if chain else 0) + tab[row * cols + c1] * a
    h %= m
    return [h, a, h]


# ---- the three calls over Python ints, a round handed the raw counter ------------------------------------------------------------
def model_walk(fn, m, na, inv, entries, n, rounds, trace=None, walk_stride=0, top=0, group=0, group_stride=0, j_base=0, j_group_step=0,
               heads=False, lanes=1):
    """vdf_round_tape_walk[_lanes]: fn(entry, J, inv, m); j_base and inv per lane when lanes > 1 (lists of `lanes`)"""
    if group == 0:
        group, group_stride = n, 0
    jb = j_base if isinstance(j_base, (list, tuple)) else [j_base]
    n_inv = len(inv) // lanes
    for w in range(n):
        G, first = w // group, (w % group) * walk_stride + top
        g, l = G // lanes, G % lanes
        cur = entries[w * na:(w + 1) * na]
        for r in range(rounds):
            k = first - r
            if trace is not None:
                trace[(G * group_stride + k) * na:(G * group_stride + k + 1) * na] = cur
            cur = fn(cur, (jb[l] + g * j_group_step + k - 1) % 2**64, inv[l * n_inv:(l + 1) * n_inv], m)
        entries[w * na:(w + 1) * na] = cur
        if trace is not None and heads and w % group == 0:
            k = first - rounds
            trace[(G * group_stride + k) * na:(G * group_stride + k + 1) * na] = cur


def model_forward(fn, m, na, inv, entries, n, rounds, checkpoints=None, every=0, cp_stride=0, trace=None, walk_stride=0, base=0,
                  j_base=0, j_walk_step=0):
    for w in range(n):
        cur = entries[w * na:(w + 1) * na]
        for r in range(rounds):
            cur = fn(cur, (j_base + w * j_walk_step + base + r) % 2**64, inv, m)
            g = base + r + 1
            if trace is not None:
                trace[(w * walk_stride + g) * na:(w * walk_stride + g + 1) * na] = cur
            if checkpoints is not None and g % every == 0:
                k = w * cp_stride + g // every
                checkpoints[k * na:(k + 1) * na] = cur
        entries[w * na:(w + 1) * na] = cur


# ---- TM: MinRoot's round with a table in the place of i --------------------------------------------------------------------------
def minroot_forward_body(field, table, c0, c1, chain_steps=None):
    """c0: a column, or None (no such term).  chain_steps: the library's own chain (pow_chain), else square-and-multiply (pow)"""
    e = pow(5, -1, MOD[field] - 1)

    def b(cs, j, inv, cur):
        s = cs.add(cur[0], cur[1])
        if c0 is not None:
            s = cs.add(s, cs.tab(table, c0))
        root = cs.pow_chain(s, chain_steps) if chain_steps else cs.pow(s, e)
        return [root, cs.add(cur[0], cs.tab(table, c1))]
    return WalkBody(0, 2, b)


def minroot_walk_body(field, table, c0, c1):
    def b(cs, j, inv, nxt):
        cx = cs.sub(nxt[1], cs.tab(table, c1))
        x2 = cs.mul(nxt[0], nxt[0])
        cy = cs.sub(cs.mul(cs.mul(x2, x2), nxt[0]), cx)
        if c0 is not None:
            cy = cs.sub(cy, cs.tab(table, c0))
        return [cx, cy]
    return WalkBody(0, 2, b)


def minroot_forward_ints(cur, J, inv, m, tab, rows, cols, c0, c1):
    x, y = cur
    row = tab_row(J, rows)
    k0 = tab[row * cols + c0] if c0 is not None else 0
    return [pow((x + y + k0) % m, pow(5, -1, m - 1), m), (x + tab[row * cols + c1]) % m]


def minroot_walk_ints(nxt, J, inv, m, tab, rows, cols, c0, c1):
    x, y = nxt
    row = tab_row(J, rows)
    cx = (y - tab[row * cols + c1]) % m
    return [cx, (pow(x, 5, m) - cx - (tab[row * cols + c0] if c0 is not None else 0)) % m]


def minroot_chain(field, tab, rows, cols, c0, c1, rounds, x0, y0=0):
    """every entry of the tabbed chain from (x0, y0): flat ints (rounds + 1) x 2, round k under J = k"""
    m = MOD[field]
    cur, out = [x0 % m, y0 % m], [x0 % m, y0 % m]
    for k in range(rounds):
        cur = minroot_forward_ints(cur, k, [], m, tab, rows, cols, c0, c1)
        out += cur
    return out


class TM(StepCircuit):
    """the circuit of examples/prove_tabbed_chain.c: z = (x, y) per lane, t rounds of TM per step.  mode 'repeat': one cs.repeat
    (cs.repeat_lanes for lanes > 1) whose body reads the table by cs.tab; mode 'loop': the plain loop with cs.const of the same
    entries -- the same shape and the same digest.  advice: a uint64 array or a device tensor set before a witness synthesis, else
    cs.step_advice() (a chain's); advice_ints: the same as ints, lane l's t + 1 entries at entry l (t + 1), for the loop."""

    def __init__(self, t, table, tab_ints, mode="repeat", field=FIELD_FQ, c0=0, c1=1, lanes=1):
        self.t, self.table, self.tab, self.mode, self.field, self.m = t, table, tab_ints, mode, field, MOD[field]
        self.rows, self.cols, self.c0, self.c1 = table.shape[0], table.shape[1], c0, c1
        self.lanes, self.arity = lanes, 2 * lanes
        self.advice, self.advice_ints = None, None

    def round(self, cs, k0, k1, carry, xn):
        x, y = carry
        t1 = cs.mul(xn, xn)
        t2 = cs.mul(t1, t1)
        cs.enforce(t2, xn, cs.add(cs.add(x, y), k0))
        return [xn, cs.add(x, k1)]

    def body(self):
        return RoundBody(0, 2, 2, lambda cs, j, inv, carry, cur, nxt: self.round(cs, cs.tab(self.table, self.c0), cs.tab(self.table, self.c1), carry,
                                                                                 cs.alloc_from(nxt[0])))

    def synthesize(self, cs, z):
        if self.mode == "repeat":
            adv = None
            if cs.is_witness:
                adv = self.advice if self.advice is not None else cs.step_advice()
            if self.lanes == 1:
                return cs.repeat(self.body(), self.t, [], list(z), adv)
            return cs.repeat_lanes(self.body(), self.t, self.lanes, [], list(z), adv)
        out = []
        for l in range(self.lanes):
            x, y = z[2 * l:2 * l + 2]
            for j in range(self.t):
                row = tab_row(j, self.rows)
                xn = cs.alloc(fe(self.advice_ints[2 * (l * (self.t + 1) + j + 1)], self.m) if cs.is_witness else None)
                x, y = self.round(cs, cs.const(fe(self.tab[row * self.cols + self.c0], self.m)),
                                  cs.const(fe(self.tab[row * self.cols + self.c1], self.m)), [x, y], xn)
            out += [x, y]
        return out
