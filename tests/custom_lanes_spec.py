"""Custom chains in lanes (include/vdf_nova.h vdf_cs_repeat_lanes, vdf_nova_custom_chain_lanes_from_checkpoints; include/vdf_hip.h
vdf_round_tape_run_lanes, vdf_round_tape_walk_lanes) for the CPU and the GPU tests: the circuit, its chains and big-integer models of
the two device calls (oracle/pasta.py integers: the reference of the host evaluators and of the kernels).

FL  L forward MinRoot chains side by side in ONE step circuit of arity 3 L, z = (x_0, y_0, i_0, x_1, y_1, i_1, ...): circuit F of
    rounds_spec per lane.  Written three ways: `repeat` through cs.repeat_lanes (advice: the host array or device tensor set on the
    circuit, else cs.step_advice() -- the circuit a lanes chain drives), `loop` as the plain double loop `for l: for j:` of the
    calls the seam always had, and `repeat1` (L = 1 only) through cs.repeat.  Lane l's advice starts lane_stride entries after
    lane l - 1's.  Lane l's chain starts at (X0 + l, 0, I0 + 1000 l)."""
import functools

import numpy as np

from rounds_spec import F, MOD, mont_rows
from custom_chain_spec import I0, X0, checkpoints_of, minroot_chain
from vdf_amd.hip import WALK_MAX_SLOTS
from vdf_amd.nova import WalkBody, record_walk_body, FIELD_FQ

MAX_LANES = 16                    # VDF_TAPE_MAX_LANES
ENFORCE_INDEX = 2                 # of F's round: mul, mul, enforce


BASE = (X0, I0)


def lane_start(l, base=BASE):
    """(x0, i0) of lane l: the lanes' roots differ, and their counters are 1000 apart"""
    return base[0] + l, base[1] + 1000 * l


class FL(F):
    def __init__(self, t, lanes, mode="repeat", field=FIELD_FQ, lane_stride=None):
        super().__init__(t, mode, field)
        self.lanes, self.arity = lanes, 3 * lanes
        self.lane_stride = t + 1 if lane_stride is None else lane_stride

    def synthesize(self, cs, z):
        L, t = self.lanes, self.t
        xy = [v for l in range(L) for v in z[3 * l:3 * l + 2]]
        inv = [z[3 * l + 2] for l in range(L)]
        if self.mode == "repeat":
            adv = None
            if cs.is_witness:
                adv = self.advice if self.advice is not None else cs.step_advice()
            xy = cs.repeat_lanes(self.body(), t, L, inv, xy, adv, self.lane_stride)
        elif self.mode == "repeat1":
            xy = cs.repeat(self.body(), t, inv, xy, self.advice if cs.is_witness else None)
        else:
            out = []
            for l in range(L):
                x, y = xy[2 * l:2 * l + 2]
                for j in range(t):
                    at = 2 * (l * self.lane_stride + j + 1)
                    xn = cs.alloc(self.fe(self.advice_ints[at]) if cs.is_witness else None)
                    x, y = self.round(cs, cs.const(self.fe(j)), [inv[l]], [x, y], xn)
                out += [x, y]
            xy = out
        tt = cs.const(self.fe(t))
        return [v for l in range(L) for v in (xy[2 * l], xy[2 * l + 1], cs.add(inv[l], tt))]


def lane_entries(field, t, steps, l, base=BASE):
    x0, i0 = lane_start(l, base)
    return minroot_chain(field, t, steps, x0, i0)


def z_of(field, lanes, t=0, steps=0, base=BASE):
    """z after `steps` steps (0: z0): 3 L elements as bytes"""
    m, out = MOD[field], []
    for l in range(lanes):
        x0, i0 = lane_start(l, base)
        e = lane_entries(field, t, steps, l, base) if steps else [x0 % m, 0]
        out += [mont_rows([v], m).tobytes() for v in (e[-2], e[-1], (i0 + steps * t) % m)]
    return out


def step_advice_ints(field, t, steps, lanes, g, lane_stride=None, base=BASE):
    """the advice of step g, flat ints: lane l's entries g t .. (g + 1) t at entry l * lane_stride (zeros in the gaps)"""
    stride = t + 1 if lane_stride is None else lane_stride
    out = [0] * (2 * ((lanes - 1) * stride + t + 1))
    for l in range(lanes):
        e = lane_entries(field, t, steps, l, base)
        out[2 * l * stride:2 * (l * stride + t + 1)] = e[2 * g * t:2 * ((g + 1) * t + 1)]
    return out


def lanes_checkpoints(field, t, steps, every, lanes, lane_stride=None, base=BASE):
    """the chains' checkpoints, lane l's steps * t / every + 1 entries at entry l * lane_stride: uint64[., 4] Montgomery"""
    m, per_lane = MOD[field], steps * (t // every) + 1
    stride = per_lane if lane_stride is None else lane_stride
    out = np.zeros(((lanes - 1) * stride + per_lane, 2, 4), dtype="<u8")
    for l in range(lanes):
        out[l * stride:l * stride + per_lane] = checkpoints_of(lane_entries(field, t, steps, l, base), 2, every, m).reshape(-1, 2, 4)
    return out.reshape(-1, 4)


def walk_inv_and_j_base(field, lanes, base=BASE):
    """per lane (inv, j_base) of walks_spec.minroot_body with inv + j_base = the lane's first counter: the counters differ per lane"""
    m = MOD[field]
    j_base = [5 * l for l in range(lanes)]
    return mont_rows([(lane_start(l, base)[1] - j_base[l]) % m for l in range(lanes)], m), j_base


# ---- big-integer models ------------------------------------------------------------------------------------------------------
def model_run_lanes(variables, adv, na, t, lanes, lane_stride, inv, n_inv, m):
    """vdf_round_tape_run_lanes over ints: `variables(adv_of_lane, t, inv_of_lane, m)` per lane, lane-major"""
    out = []
    for l in range(lanes):
        out += variables(adv[l * lane_stride * na:(l * lane_stride + t + 1) * na], t, inv[l * n_inv:(l + 1) * n_inv], m)
    return out


def model_walk_lanes(fn, m, na, lanes, inv, n_inv, entries, n, rounds, trace=None, walk_stride=0, top=0, group=0, group_stride=0, j_base=None,
                     j_group_step=0, heads=False):
    """The contract of vdf_round_tape_walk_lanes over Python ints (walks_spec.model_walk with the groups numbered step-major,
    lane-minor): entries (flat, n x na) and trace (flat list, or None) in place."""
    j_base = [0] * lanes if j_base is None else j_base
    if group == 0:
        group, group_stride = n, 0
    for w in range(n):
        G, first = w // group, (w % group) * walk_stride + top
        g, l = G // lanes, G % lanes
        cur = entries[w * na:(w + 1) * na]
        for r in range(rounds):
            k = first - r
            if trace is not None:
                assert k >= 0
                trace[(G * group_stride + k) * na:(G * group_stride + k + 1) * na] = cur
            j = (j_base[l] + g * j_group_step + k - 1) % 2**64
            cur = fn(cur, j % m, inv[l * n_inv:(l + 1) * n_inv], m)
        entries[w * na:(w + 1) * na] = cur
        if trace is not None and heads and w % group == 0:
            k = first - rounds
            assert k >= 0
            trace[(G * group_stride + k) * na:(G * group_stride + k + 1) * na] = cur


@functools.lru_cache(maxsize=None)
def every_op_lanes_chain(field, t, steps, every, lanes, wrap_lane=1):
    """`lanes` chains of walks_spec's three-column body, each built downwards from a random last entry (0, 1 and m - 1 among the last
    entries): (inv ints per lane, j_base per lane, checkpoints[l] flat ints of steps * t / every + 1 entries).  The lanes' inv are all
    distinct, and lane `wrap_lane` counts from 2^64 - 12, so that its counter wraps inside the first step."""
    from walks_spec import every_op_ints, start_entries
    m, per = MOD[field], t // every
    inv = [99 + 7 * l for l in range(lanes)]
    j_base = [1000 * l for l in range(lanes)]
    if lanes > wrap_lane:
        j_base[wrap_lane] = 2**64 - 12
    tops = start_entries(lanes, 3, m, np.random.default_rng(11 + field + lanes))
    cps = []
    for l in range(lanes):
        cur, mine = list(tops[3 * l:3 * l + 3]), []
        for k in range(steps * t, 0, -1):
            if k % every == 0:
                mine.insert(0, list(cur))
            cur = every_op_ints(cur, ((j_base[l] + k - 1) % 2**64) % m, [inv[l]], m)
        mine.insert(0, list(cur))
        cps.append([v for c in mine for v in c])
    assert len(cps[0]) == 3 * (steps * per + 1)
    return inv, j_base, cps


def window_walks(cps, lanes, per, first, count, na=3):
    """the walks of steps [first, first + count) in the order of vdf_round_tape_walk_lanes (step-major, lane-minor): the entries the
    walks stand on and the checkpoints they must land on, flat ints"""
    starts, expect = [], []
    for g in range(first, first + count):
        for l in range(lanes):
            starts += cps[l][(g * per + 1) * na:(g * per + 1 + per) * na]
            expect += cps[l][g * per * na:(g * per + per) * na]
    return starts, expect


# ---- a walk tape at the slot cap of the walk in lanes ---------------------------------------------------------------------------
def wide_walk(n_live, n_adv, n_inv):
    def b(c, j, inv, nxt):
        a = [c.add(nxt[0], inv[n_inv - 1])]
        for _ in range(n_live - 1):
            a.append(c.add(a[-1], a[-1]))
        s = a[0]
        for x in a[1:]:
            s = c.add(s, x)
        return [s] * n_adv
    return WalkBody(n_inv, n_adv, b)


def walk_at_the_slot_cap(na=5, n_inv=2):
    """a walk tape with n_slots + 2 n_adv + n_inv = VDF_WALK_MAX_SLOTS exactly"""
    for n_live in range(2, WALK_MAX_SLOTS):
        tape = record_walk_body(wide_walk(n_live, na, n_inv))
        if tape.c.n_slots + 2 * na + n_inv == WALK_MAX_SLOTS:
            return tape
    raise AssertionError("no body reaches the cap")
