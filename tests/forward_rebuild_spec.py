"""Traces rebuilt by forward tapes (include/vdf_hip.h vdf_round_tape_rebuild_lanes; include/vdf_nova.h
vdf_nova_forward_tape_rebuild_eval_lanes and the ascending vdf_custom_chain) for the CPU and the GPU tests.

THE ORACLE is independent of the new index rule: one whole chain per lane, walked from entry 0 by the existing host evaluator
(nova.forward_tape_eval, one walk, trace on, VDF_TAPE_J = the lane's j_base + the index of the entry stood on, modulo 2^64).  Step
g's trace is chain entries g t .. g t + t; the walk of interval m of that step starts on entry g t + m every and must land on
entry g t + (m + 1) every.  What a window of a rebuild call must leave in `trace`, `entries` and `ok` is cut from those chains.

X   a forward body of na columns that uses every op a forward tape may hold, with one invariant k (so that lanes differ):
      d = cur[0] + cur[na - 1] - k + j (+ tab[0]);  out[0] = d^5 (POW) + cur[1]^5 (POWC) * (tab[1] or 3);  out[i] = cur[i - 1] + i.
R   a two-element Rescue-shaped round.  State (s0, s1), M = [[2, 1], [1, 3]], round constants (c0, c1) = table[J mod rows]:
      root layer   r_i = s_i^(1/5)
      mix, add     (a0, a1) = M (r0, r1) + (c0, c1)
      power layer  p_i = a_i^5
      mix          (s0', s1') = M (p0, p1)
    Both directions need a 254-bit exponentiation: no walk tape exists.  An entry is (s0, s1, r0, r1) -- the state, and the two roots
    that PRODUCED it -- so the round body relating entries j and j + 1 needs only products: it allocates r_i from entry j + 1,
    enforces r_i^5 = s_i against its carry, and carries M (M r + c)^5 out."""
import itertools

import numpy as np

from rounds_spec import MOD, fe, mont_rows
from util import ints
from vdf_amd.minroot import pow_chain as minroot_pow_chain
from vdf_amd.nova import RoundBody, StepCircuit, WalkBody, forward_tape_eval, record_forward_body, FIELD_FP, FIELD_FQ

CHAIN5 = [(0, 2, 0, 0xFF)]             # x -> x^5: from T[0], two squarings, times T[0]
FILL = 0xA5A5A5A5A5A5A5A5              # every word of an element nothing may write
FORWARD_TAPE_MAX_WORK = 1 << 20
WALK_MAX_SLOTS, TAPE_MAX_LANES, TAPE_MAX_INV = 32, 16, 16


# ---- X ---------------------------------------------------------------------------------------------------------------------------
def every_op_body(field, na, table=None):
    m = MOD[field]

    def b(cs, j, inv, cur):
        d = cs.add(cs.sub(cs.add(cur[0], cur[na - 1]), inv[0]), j)
        if table is not None:
            d = cs.add(d, cs.tab(table, 0))
        k = cs.tab(table, 1) if table is not None else cs.const(fe(3, m))
        out = [cs.add(cs.pow(d, 5), cs.mul(cs.pow_chain(cur[1], CHAIN5), k))]
        for i in range(1, na):
            out.append(cs.add(cur[i - 1], cs.const(fe(i, m))))
        return out
    return WalkBody(1, na, b)


def every_op_ints(cur, J, inv, m, na, tab=None, rows=0, cols=0):
    row = (J % 2**64) % rows if tab is not None else 0
    d = (cur[0] + cur[na - 1] - inv[0] + J + (tab[row * cols] if tab is not None else 0)) % m
    k = tab[row * cols + 1] if tab is not None else 3
    return [(pow(d, 5, m) + pow(cur[1], 5, m) * k) % m] + [(cur[i - 1] + i) % m for i in range(1, na)]


# ---- R ---------------------------------------------------------------------------------------------------------------------------
def rescue_forward_body(field, table, wrong=False):
    """wrong: the second mix adds 1 to s0' -- a forward tape that disagrees with the round body"""
    m, root = MOD[field], minroot_pow_chain(field)

    def b(cs, j, inv, cur):
        r0, r1 = cs.pow_chain(cur[0], root), cs.pow_chain(cur[1], root)
        a0 = cs.add(cs.add(cs.scale(r0, fe(2, m)), r1), cs.tab(table, 0))
        a1 = cs.add(cs.add(r0, cs.scale(r1, fe(3, m))), cs.tab(table, 1))
        p = []
        for a in (a0, a1):
            q = cs.mul(a, a)
            p.append(cs.mul(cs.mul(q, q), a))
        s0 = cs.add(cs.scale(p[0], fe(2, m)), p[1])
        if wrong:
            s0 = cs.add(s0, cs.const(fe(1, m)))
        return [s0, cs.add(p[0], cs.scale(p[1], fe(3, m))), r0, r1]
    return WalkBody(0, 4, b)


def rescue_forward_ints(cur, J, m, tab, rows):
    e = pow(5, -1, m - 1)
    row = (J % 2**64) % rows
    r0, r1 = pow(cur[0], e, m), pow(cur[1], e, m)
    p0, p1 = pow((2 * r0 + r1 + tab[2 * row]) % m, 5, m), pow((r0 + 3 * r1 + tab[2 * row + 1]) % m, 5, m)
    return [(2 * p0 + p1) % m, (p0 + 3 * p1) % m, r0, r1]


def rescue_round_body(field, table):
    m = MOD[field]

    def b(cs, j, inv, carry, cur, nxt):
        r = []
        for i in range(2):                             # (the order of examples/prove_rescue_chain.c: the same shape and digest)
            r.append(cs.alloc_from(nxt[2 + i]))
            t1 = cs.mul(r[i], r[i])
            cs.enforce(cs.mul(t1, t1), r[i], carry[i])
        a0 = cs.add(cs.add(cs.scale(r[0], fe(2, m)), r[1]), cs.tab(table, 0))
        a1 = cs.add(cs.add(r[0], cs.scale(r[1], fe(3, m))), cs.tab(table, 1))
        p = []
        for a in (a0, a1):
            q = cs.mul(a, a)
            p.append(cs.mul(cs.mul(q, q), a))
        return [cs.add(cs.scale(p[0], fe(2, m)), p[1]), cs.add(p[0], cs.scale(p[1], fe(3, m)))]
    return RoundBody(0, 2, 4, b)


def rescue_table(field, rows):
    """row r = (1000 + 7 r, 1 + r^2): (flat ints, the uint64[rows, 2, 4] Montgomery array)"""
    m = MOD[field]
    vals = [v for r in range(rows) for v in (1000 + 7 * r, 1 + r * r)]
    return vals, np.ascontiguousarray(mont_rows(vals, m).reshape(rows, 2, 4))


class Rescue(StepCircuit):
    """z = (s0, s1) per lane, t rounds of R per step in one cs.repeat (cs.repeat_lanes for lanes > 1).  advice: a uint64 array or a
    device tensor set before a witness synthesis, else cs.step_advice() (a chain's)."""

    def __init__(self, t, table, field=FIELD_FQ, lanes=1, probe=None):
        self.t, self.table, self.field, self.lanes, self.arity = t, table, field, lanes, 2 * lanes
        self.advice, self.probe = None, probe      # probe: called once per proved step (a witness synthesis that is no lookahead's)

    def synthesize(self, cs, z):
        adv = None
        if cs.is_witness and not cs.is_probe and self.probe is not None:
            self.probe()
        if cs.is_witness:
            adv = self.advice if self.advice is not None else cs.step_advice()
        body = rescue_round_body(self.field, self.table)
        if self.lanes == 1:
            return cs.repeat(body, self.t, [], list(z), adv)
        return cs.repeat_lanes(body, self.t, self.lanes, [], list(z), adv)


# ---- the oracle: whole chains, and what a window is cut from them ----------------------------------------------------------------
def chain_trace(field, tape, inv, start, rounds, j_base=0, cut=64):
    """entries 0 .. rounds of ONE chain from `start` (uint64[na, 4]) by the host's forward evaluator, in calls of at most `cut`
    rounds: uint64[(rounds + 1) * na, 4]"""
    na = tape.c.n_adv
    e = np.ascontiguousarray(start, dtype="<u8").reshape(na, 4).copy()
    tr = np.zeros(((rounds + 1) * na, 4), dtype="<u8")
    tr[:na] = e
    done = 0
    while done < rounds:
        now = min(cut, rounds - done)
        forward_tape_eval(field, tape, inv, e, 1, now, trace=tr, walk_stride=0, base=done, j_base=j_base % 2**64)
        done += now
    return tr


def lane_chains(field, tape, lanes, n_inv, inv, starts, rounds, j_base):
    """one chain per lane: inv uint64[lanes * n_inv, 4] or None, starts uint64[lanes * na, 4], j_base a list of `lanes` ints"""
    na = tape.c.n_adv
    return [chain_trace(field, tape, None if not n_inv else inv[l * n_inv:(l + 1) * n_inv], starts[l * na:(l + 1) * na], rounds, j_base[l])
            for l in range(lanes)]


def window(chains, na, t, every, first, count):
    """the walks of steps [first, first + count), step-major, lane-minor: (starts below, targets above), uint64[walks * na, 4] each"""
    per, lo, hi = t // every, [], []
    for g in range(first, first + count):
        for c in chains:
            for mth in range(per):
                k = g * t + mth * every
                lo.append(c[k * na:(k + 1) * na])
                hi.append(c[(k + every) * na:(k + every + 1) * na])
    return np.concatenate(lo), np.concatenate(hi)


def window_traces(chains, na, t, first, count, group_stride, heads=True, total=None):
    """what the launches of the window leave in a trace array that held FILL: group G = li * lanes + l at G * group_stride, entries
    1 .. t (0 .. t with heads); uint64[total or count * lanes * group_stride, na * 4]"""
    lanes = len(chains)
    out = np.full((total or count * lanes * group_stride, na * 4), FILL, dtype="<u8")
    for li in range(count):
        for l, c in enumerate(chains):
            G, k0 = li * lanes + l, (first + li) * t
            lo = 0 if heads else 1
            out[G * group_stride + lo:G * group_stride + t + 1] = c.reshape(-1, na * 4)[k0 + lo:k0 + t + 1]
    return out.reshape(-1, 4)


def step_advice(chains, na, t, g):
    """step g's advice: lane l's entries g t .. g t + t at entry l (t + 1)"""
    return np.concatenate([c[g * t * na:(g * t + t + 1) * na] for c in chains])


def tape_ints(arr, m):
    from oracle import pasta as o
    return [o.from_mont(v, m) for v in ints(arr)]


# ---- the matrix both test files run: every = 5 cut into 2 + 2 + 1, two steps, a table of 3 rows ---------------------------------------
EVERY, SLICES, STEPS, ROWS = 5, (2, 2, 1), 2, 3
MATRIX = list(itertools.product((FIELD_FQ, FIELD_FP), (2, 4), (1, 3), (2, 4), (0, 1), (False, True)))
IDS = ["%s na=%d L=%d group=%d heads=%d %s" % ("Fq" if f == FIELD_FQ else "Fp", na, L, g, h, "tab" if tab else "plain") for f, na, L, g, h, tab in MATRIX]


def case(field, na, lanes, group, tab):
    """(tape, inv, j_base per lane, the lanes' chains, t) of one cell of the matrix: j_base = 2^64 - 3 in lane 0, so that J wraps"""
    m, t = MOD[field], group * EVERY
    table = None
    if tab:
        vals = [11 + 5 * r + c for r in range(ROWS) for c in range(2)]
        table = np.ascontiguousarray(mont_rows(vals, m).reshape(ROWS, 2, 4))
    tape = record_forward_body(every_op_body(field, na, table), field)
    inv = mont_rows([9 + 1000 * l for l in range(lanes)], m)
    jb = [(2**64 - 3 + 1000 * l) % 2**64 for l in range(lanes)]
    starts = mont_rows([0, 1, m - 1] + [int(v) for v in np.random.default_rng(na + lanes).integers(1, 2**62, size=lanes * na)][:lanes * na - 3], m)
    chains = lane_chains(field, tape, lanes, 1, inv, starts, STEPS * t, jb)
    return tape, inv, jb, chains, t


def run_window(call, field, tape, lanes, inv, jb, lo, hi, trace, ok, t, group, heads, group_stride):
    """the launches of one window: slices of 2 + 2 + 1 rounds, the comparison in the last"""
    entries, base = lo.copy(), 0
    for i, now in enumerate(SLICES):
        last = i == len(SLICES) - 1
        call(field, tape, lanes, inv, entries, len(ok), now, trace=trace, walk_stride=EVERY, base=base, group=group, group_stride=group_stride,
             j_base=jb, j_group_step=t, heads=heads, expect=hi if last else None, ok=ok if last else None)
        base += now
    return entries
