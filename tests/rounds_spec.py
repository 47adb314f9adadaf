"""The two test circuits of the repeated-rounds seam (include/vdf_nova.h vdf_cs_repeat), each written twice -- through
`cs.repeat` and as a plain loop of the calls the seam always had -- with their advice and a big-integer interpretation of
their variables (oracle/pasta.py integers: the reference of the host evaluator and of the kernel).

F  the forward MinRoot round (src/minroot.rs:329-335 in the direction of evaluation): arity 3, z = (x, y, i); carry (x, y),
   inv = (i_in); per round xn = alloc_from(next[0]), t1 = xn^2, t2 = t1^2, t2 * xn = x + y enforced, yn = x + i_in + j.
   Advice: a vdf_minroot_eval trace (n_adv = 2).  z_out = (x_t, y_t, i_in + t).
G  a round that uses every op: arity 2, z = (a, k); carry (a), inv = (k), n_adv = 3 with columns (a_j, u_j, w_j):
     u = alloc_from(cur[1]); w = alloc_from(3 * (next[2] - cur[2])); p = u * w; s = p - 7 a + (j + 11); q = s * s; r = q * k;
     q * k = r enforced once more; a' = r + u.
   Advice is made here: u, w free, a_(j+1) by the recurrence.  z_out = (a_t, k)."""
import numpy as np

from oracle import pasta as o
from util import limbs
from vdf_amd.nova import RoundBody, StepCircuit, FIELD_FQ

MOD = {o.FIELD_FP: o.P, o.FIELD_FQ: o.Q}


def fe(v, m):
    return limbs([o.to_mont(v % m, m)]).tobytes()


def mont_rows(vals, m):
    """ints -> uint64[n, 4] Montgomery"""
    return limbs([o.to_mont(v % m, m) for v in vals])


class _Rounds(StepCircuit):
    """mode: 'repeat' or 'loop'.  advice: set before every witness synthesis -- a uint64 array (host), or a device tensor
    (repeat only); advice_ints: the same as Python ints, flat entry-major (what the plain loop allocates from)."""

    def __init__(self, t, mode, field=FIELD_FQ):
        self.t, self.mode, self.field, self.m = t, mode, field, MOD[field]
        self.advice, self.advice_ints = None, None
        self.repeat_rc = []

    def fe(self, v):
        return fe(v, self.m)


class F(_Rounds):
    arity, n_adv, n_vars = 3, 2, 3

    def round(self, cs, j, inv, carry, xn):
        """the calls of one round, the same in both forms; xn: the new root's variable"""
        x, y = carry
        t1 = cs.mul(xn, xn)
        t2 = cs.mul(t1, t1)
        cs.enforce(t2, xn, cs.add(x, y))
        yn = cs.add(cs.add(x, inv[0]), j)
        return [xn, yn]

    def body(self):
        return RoundBody(1, 2, 2, lambda cs, j, inv, carry, cur, nxt: self.round(cs, j, inv, carry, cs.alloc_from(nxt[0])))

    def synthesize(self, cs, z):
        x, y, i_in = z
        if self.mode == "repeat":
            x, y = cs.repeat(self.body(), self.t, [i_in], [x, y], self.advice if cs.is_witness else None)
        else:
            for j in range(self.t):
                xn = cs.alloc(self.fe(self.advice_ints[2 * (j + 1)]) if cs.is_witness else None)
                x, y = self.round(cs, cs.const(self.fe(j)), [i_in], [x, y], xn)
        return [x, y, cs.add(i_in, cs.const(self.fe(self.t)))]

    @staticmethod
    def variables(adv, t, inv, m):
        """big-int interpretation: the 3t variables from the advice alone"""
        out = []
        for j in range(t):
            xn = adv[2 * (j + 1)]
            out += [xn, xn * xn % m, pow(xn, 4, m)]
        return out


class G(_Rounds):
    arity, n_adv, n_vars = 2, 3, 5

    def round(self, cs, j, inv, carry, u, w):
        p = cs.mul(u, w)
        s = cs.sub(p, cs.scale(carry[0], self.fe(7)))
        s = cs.add(s, cs.add(j, cs.const(self.fe(11))))
        q = cs.mul(s, s)
        r = cs.mul(q, inv[0])
        cs.enforce(q, inv[0], r)
        return [cs.add(r, u)]

    def body(self):
        def b(cs, j, inv, carry, cur, nxt):
            u = cs.alloc_from(cur[1])
            w = cs.alloc_from(cs.scale(cs.sub(nxt[2], cur[2]), self.fe(3)))
            return self.round(cs, j, inv, carry, u, w)
        return RoundBody(1, 1, 3, b)

    def synthesize(self, cs, z):
        a, k = z
        if self.mode == "repeat":
            (a,) = cs.repeat(self.body(), self.t, [k], [a], self.advice if cs.is_witness else None)
        else:
            A = self.advice_ints
            for j in range(self.t):
                wit = cs.is_witness
                u = cs.alloc(self.fe(A[3 * j + 1]) if wit else None)
                w = cs.alloc(self.fe(3 * (A[3 * (j + 1) + 2] - A[3 * j + 2])) if wit else None)
                (a,) = self.round(cs, cs.const(self.fe(j)), [k], [a], u, w)
        return [a, k]

    @staticmethod
    def variables(adv, t, inv, m):
        out = []
        for j in range(t):
            a, u = adv[3 * j], adv[3 * j + 1]
            w = 3 * (adv[3 * (j + 1) + 2] - adv[3 * j + 2]) % m
            p = u * w % m
            s = (p - 7 * a + j + 11) % m
            q = s * s % m
            out += [u, w, p, q, q * inv[0] % m]
        return out

    @staticmethod
    def advice_for(a0, k, t, m, rng, special=()):
        """consistent advice: free u, w (the first of them `special`), a by the recurrence; flat ints, (t + 1) x 3"""
        free = list(special) + [int(rng.integers(0, 2**62)) ** 4 % m for _ in range(2 * (t + 1))]
        us, ws = free[:t + 1], free[t + 1:2 * (t + 1)]
        adv, a = [], a0 % m
        for j in range(t + 1):
            adv += [a, us[j], ws[j]]
            if j < t:
                w = 3 * (ws[j + 1] - ws[j]) % m
                s = (us[j] * w - 7 * a + j + 11) % m
                a = (s * s * k + us[j]) % m
        return adv


def minroot_advice(x, y, i, t, field):
    """F's advice by the oracle's evaluator: flat ints (t + 1) x 2, and the final state"""
    m = MOD[field]
    adv, s = [x % m, y % m], o.State(x % m, y % m, i % m)
    for _ in range(t):
        s = o.minroot_eval(s, 1, field)
        adv += [s.x, s.y]
    return adv, s
