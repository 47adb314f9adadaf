"""Caller-supplied addition chains (include/vdf_hip.h vdf_pow_step, VDF_TAPE_POWC; include/vdf_nova.h vdf_cs_pow_chain,
vdf_nova_pow_chain_exponent, vdf_nova_pow_chain_window, vdf_minroot_pow_chain) for the CPU and the GPU tests: an integer model of a
chain (its value over Python ints modulo m, and its exponent), a restatement of the sliding-window generator, and the test bodies.

A chain is a list of steps (src, squarings, mul, dst) over an accumulator v and temporaries T, T[0] the base:
    v = T[src] unless src == ACC;  v = v^(2^squarings);  v = v * T[mul] unless mul == NONE;  T[dst] = v unless dst == NONE
The oracle of the whole feature: a POWC of a chain with exponent E is byte for byte a POW of E.

M  the MinRoot forward round of forward_tape_spec with its root taken by a chain.
E  forward_tape_spec's body of every op and six powers with some of the powers ALSO taken by a window chain and the two results
   added.  All five exponents >= 1 at window 3 take 21 packed constants, which with the body's own 8 is beyond the 24 a tape holds
   (VDF_ROUND_MAX_CONSTS), so the powers are spread over two bodies: EVERY_OP_CHAINS_A takes exponents 1, 2, 2^255 and m - 2 by
   window-3 chains, EVERY_OP_CHAINS_B takes 2^255 - 1 by a window-3 chain (88 steps, 12 constants, 5 temporaries) and exponent 1 by
   a window-2 chain (3 temporaries): a POW and two POWC of different n_tmp in one tape."""
from rounds_spec import MOD, fe
from forward_tape_spec import every_op_exponents, root_exponent
from vdf_amd.nova import WalkBody

ACC, NONE = 0xFE, 0xFF
MAX_STEPS, MAX_TMP = 95, 12
TAPE_POWC = 10


def run_chain(steps, x, m):
    """(value mod m, exponent) of the chain over base x: both by the steps alone"""
    T, E = {0: x % m}, {0: 1}
    v = e = None
    for src, sq, mul, dst in steps:
        if src != ACC:
            v, e = T[src], E[src]
        v, e = pow(v, 2**sq, m), e << sq
        if mul != NONE:
            v, e = v * T[mul] % m, e + E[mul]
        if dst != NONE:
            T[dst], E[dst] = v, e
    return v, e


def chain_exponent(steps):
    return run_chain(steps, 1, 3)[1]


def chain_tmp(steps):
    """the temporaries a chain needs: its largest index + 1"""
    return 1 + max([0] + [k for s in steps for k in (s[0], s[2], s[3]) if k < ACC])


def chain_products(steps):
    """what the header counts for a POWC"""
    return max(1, sum(s[1] for s in steps) + sum(1 for s in steps if s[2] != NONE))


def packed_consts(steps):
    return (4 + 4 * len(steps) + 31) // 32


def window_chain(e, window):
    """vdf_nova_pow_chain_window restated: the table T[1] = x^2, T[1 + k] = x^(2k + 1) first and whole, then one step per window,
    left to right; windows begin and end in a one and are at most `window` bits long"""
    assert e >= 1 and 2 <= window <= 4
    steps = [(0, 1, NONE, 1)] + [(ACC, 0, 0 if k == 1 else 1, 1 + k) for k in range(1, 2**(window - 1))]
    slot = lambda odd: 0 if odd == 1 else (odd + 1) // 2
    src, pending, first, i = ACC, 0, True, e.bit_length() - 1
    while i >= 0:
        if not (e >> i) & 1:
            pending, i = pending + 1, i - 1
            continue
        lo = max(i - window + 1, 0)
        while not (e >> lo) & 1:
            lo += 1
        val = (e >> lo) & ((1 << (i - lo + 1)) - 1)
        if first:
            src, first = slot(val), False
        else:
            steps.append((src, pending + i - lo + 1, slot(val), NONE))
            src, pending = ACC, 0
        i = lo - 1
    if pending or src != ACC:
        steps.append((src, pending, NONE, NONE))
    return steps


def tmp_chain(n_tmp):
    """x^4 through T[n_tmp - 1]: a valid chain of exactly n_tmp temporaries (n_tmp >= 2), 1 squaring and 1 product"""
    return [(0, 1, NONE, n_tmp - 1), (ACC, 0, n_tmp - 1, NONE)]


def minroot_chain_body(field, steps):
    def b(cs, j, inv, cur):
        return [cs.pow_chain(cs.add(cur[0], cur[1]), steps), cs.add(cur[0], j)]
    return WalkBody(0, 2, b)


# (index into every_op_exponents, window) of the powers a body also takes by a chain
EVERY_OP_CHAINS_A = ((1, 3), (2, 3), (3, 3), (5, 3))
EVERY_OP_CHAINS_B = ((4, 3), (1, 2))


def every_op_chain_body(field, chains):
    m = MOD[field]
    E = every_op_exponents(m)

    def b(cs, j, inv, cur):
        d = cs.sub(cs.add(cur[0], cur[1]), inv[0])
        e = cs.mul(d, cur[2])
        g = cs.scale(cs.mul(e, e), fe(7, m))
        h = cs.add(cs.add(g, cs.const(fe(11, m))), j)
        bases = (g, d, cur[2], cur[0], cur[1], e)
        for base, ex in zip(bases, E):
            h = cs.add(h, cs.pow(base, ex))
        for k, window in chains:
            h = cs.add(h, cs.pow_chain(bases[k], window_chain(E[k], window)))
        return [h, cur[0], h]
    return WalkBody(1, 3, b)


def every_op_chain_ints(chains):
    def f(cur, j, inv, m):
        a, b, c = cur
        d = (a + b - inv[0]) % m
        e = d * c % m
        g = 7 * e * e % m
        E, bases = every_op_exponents(m), (g, d, c, a, b, e)
        h = g + 11 + j + sum(pow(base, ex, m) for base, ex in zip(bases, E))
        h += sum(pow(bases[k], E[k], m) for k, _ in chains)
        h %= m
        return [h, a, h]
    return f


def cases(field):
    """every chain the tests use, by name: each is checked against pow(x, E, m) by test_pow_chain_host"""
    m = MOD[field]
    out = {"tmp%d" % n: tmp_chain(n) for n in (2, 11, 12)}
    for w in (2, 3, 4):
        out["root w%d" % w] = window_chain(root_exponent(field), w)
    for k, w in EVERY_OP_CHAINS_A + EVERY_OP_CHAINS_B:
        out["every-op %d w%d" % (k, w)] = window_chain(every_op_exponents(m)[k], w)
    return out
