"""A custom circuit's chain (include/vdf_nova.h vdf_custom_chain) for the CPU and the GPU tests: the circuits, the chains and a
big-integer model of the window vdf_nova_custom_chain_materialize lays out.

FC  circuit F of rounds_spec (the forward MinRoot round, two advice columns (x, y)) taking its advice from cs.step_advice() when no
    host advice is set: the circuit a chain drives.  Its walk body is walks_spec.minroot_body: inv = (the chain's starting
    counter), VDF_TAPE_J chain-global.
FW  the same circuit with a round body that DISAGREES with the chain: x'^5 = x + y + 1 is enforced.  Every walk lands on its
    checkpoint, and constraint 2 of every repetition is unsatisfied.
E   the three-column body of walks_spec (every op), for windows of an entry that is not a MinRoot state.

Entry k of a MinRoot chain is the (x, y) of the state after k rounds; step g's trace is entries g t .. (g + 1) t."""
import functools

import numpy as np

from oracle import pasta as o
from rounds_spec import F, MOD, mont_rows
from walks_spec import every_op_body, every_op_ints, minroot_body, minroot_ints, model_walk, start_entries   # noqa: F401
from vdf_amd.nova import RoundBody, FIELD_FP, FIELD_FQ

ENFORCE_INDEX = 2                 # of F's round: mul, mul, enforce
X0, I0 = 0x51DE, 7                # where the MinRoot chains of these tests start


class FC(F):
    def synthesize(self, cs, z):
        x, y, i_in = z
        adv = None
        if cs.is_witness:
            adv = self.advice if self.advice is not None else cs.step_advice()
        self.seen.append((cs.is_witness, cs.step_advice()))
        if self.probe is not None and cs.is_witness:
            self.probe()
        x, y = cs.repeat(self.body(), self.t, [i_in], [x, y], adv)
        return [x, y, cs.add(i_in, cs.const(self.fe(self.t)))]

    def __init__(self, t, field=FIELD_FQ, probe=None):
        super().__init__(t, "repeat", field)
        self.seen, self.probe = [], probe


class FW(FC):
    def round(self, cs, j, inv, carry, xn):
        x, y = carry
        t1 = cs.mul(xn, xn)
        t2 = cs.mul(t1, t1)
        cs.enforce(t2, xn, cs.add(cs.add(x, y), cs.const(self.fe(1))))
        yn = cs.add(cs.add(x, inv[0]), j)
        return [xn, yn]


@functools.lru_cache(maxsize=None)
def minroot_chain(field, t, steps, x0=X0, i0=I0):
    """every entry of a MinRoot chain of steps * t rounds from (x0, 0, i0): flat ints (steps * t + 1) x 2, by the oracle's evaluator"""
    m = MOD[field]
    adv, s = [x0 % m, 0], o.State(x0 % m, 0, i0)
    for _ in range(steps * t):
        s = o.minroot_eval(s, 1, field)
        adv += [s.x, s.y]
    return adv


def checkpoints_of(entries_ints, na, every, m):
    """the entries every `every` rounds as uint64[., 4] Montgomery"""
    n = len(entries_ints) // na
    return mont_rows([v for k in range(0, n, every) for v in entries_ints[k * na:(k + 1) * na]], m)


def z0_of(field, x0=X0, i0=I0):
    m = MOD[field]
    return [mont_rows([v], m).tobytes() for v in (x0 % m, 0, i0)]


def zi_of(field, t, steps, x0=X0, i0=I0):
    m = MOD[field]
    e = minroot_chain(field, t, steps, x0, i0)
    return [mont_rows([v], m).tobytes() for v in (e[-2], e[-1], (i0 + steps * t) % m)]


def step_traces(field, t, steps, x0=X0, i0=I0):
    """the host advice of every step: uint64[2 (t + 1), 4] Montgomery, entries g t .. (g + 1) t"""
    m = MOD[field]
    e = minroot_chain(field, t, steps, x0, i0)
    return [mont_rows(e[2 * g * t:2 * ((g + 1) * t + 1)], m) for g in range(steps)]


def forward_minroot_body(field):
    """the slow direction of the same round, for Context.round_tape_eval_batch: x' = (x + y)^(1/5), y' = x + i0 + j"""
    from vdf_amd.nova import WalkBody
    e = pow(5, -1, MOD[field] - 1)
    return WalkBody(1, 2, lambda cs, j, inv, cur: [cs.pow(cs.add(cur[0], cur[1]), e), cs.add(cur[0], cs.add(inv[0], j))])


def model_window(fn, m, na, inv, cp_ints, first, count, t, every, j_base=0):
    """Big-integer model of a materialised window: the traces of steps [first, first + count) back to back, (t + 1) entries each,
    from the chain's checkpoints cp_ints (flat, entry-major) -- one walk of `every` rounds per checkpoint interval, the first walk
    of a step also writing its landing; and whether every walk of a step lands on the checkpoint below it."""
    per = t // every
    walks = count * per
    entries = list(cp_ints[(first * per + 1) * na:(first * per + 1 + walks) * na])
    trace = [None] * (count * (t + 1) * na)
    model_walk(fn, m, na, inv, entries, walks, every, trace, walk_stride=every, top=every, group=per, group_stride=t + 1,
               j_base=(j_base + first * t) % 2**64, j_group_step=t, heads=True)
    expect = cp_ints[first * per * na:(first * per + walks) * na]
    ok = [entries[w * na:(w + 1) * na] == list(expect[w * na:(w + 1) * na]) for w in range(walks)]
    return trace, [all(ok[g * per:(g + 1) * per]) for g in range(count)]


def every_op_chain(field, t, steps, every, j_base, seed=3):
    """checkpoints (flat ints) of a chain of the three-column body, built downwards from a random last entry: entry k - 1 is the
    body applied to entry k with j = j_base + k - 1"""
    m = MOD[field]
    inv = [99]
    per = t // every
    top = start_entries(1, 3, m, np.random.default_rng(seed))
    cps = [list(top)]
    for c in range(steps * per, 0, -1):
        cur = list(cps[0])
        for k in range(c * every, (c - 1) * every, -1):
            cur = every_op_ints(cur, ((j_base + k - 1) % 2**64) % m, inv, m)
        cps.insert(0, cur)
    return inv, [v for c in cps for v in c]
