"""Operand lists for the generated column scans (vdf_amd/csrc/fe_{mul,sqr,mul2}_gfx950.inc) and the bridge to the integer model
of their emitted schedule (tools/gen_fe_mul.py: schedule(), model()).  Shared by tests/test_fe_scan_model.py (no device) and
tests/test_gpu_fe_scan.py.  The scans assume nothing about their operands beyond 256 bits, so every list goes to every body.

The crafted lists aim at the carry adds the generator dropped: those sit behind the reduction products q_k * m_j, so the
operands are chosen to make every quotient digit q_k = 0xFFFFFFFF at once (T = -q m mod 2^256 with q = 2^256 - 1, i.e.
T = m mod 2^256: a = m with b = 1, a = m / b for odd b, a square root of m, and a = (m - c d) / b for the pair), and
every q_k = 0 (T = 0 mod 2^256), next to all-ones limbs and top limbs on both sides of 2^31."""
import importlib.util
import os
import random

import numpy as np

import prim_spec as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_fe_mul", os.path.join(ROOT, "tools", "gen_fe_mul.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

R, MASK = s.R, s.MASK
ARITY = {"mul": 2, "sqr": 1, "mul2": 4}
ONES = MASK                                  # all limbs 0xFFFFFFFF


def T_of(body, t):
    return t[0] * t[1] if body == "mul" else t[0] * t[0] if body == "sqr" else t[0] * t[1] + t[2] * t[3]


def sqrt_mod_R(v):
    """the four square roots of v = 1 (mod 8) modulo 2^256"""
    assert v % 8 == 1
    x = 1
    for k in range(3, 256):
        if (x * x - v) % (1 << (k + 1)):
            x += 1 << (k - 1)
    assert (x * x - v) % R == 0
    return sorted({x % R, -x % R, (x + (1 << 255)) % R, (-x + (1 << 255)) % R})


def edge_operands(F):
    m, top = F.m, s.lazy_top(F)
    v = [0, 1, m - 1, m, 2 * m - 1, 2 * m, top - 1, top, 3 * m, ONES, ONES - 1, ONES >> 1, 1 << 255, (1 << 255) - 1]
    # the top limb on both sides of 2^31 (the largest a lazy value has), over all-ones, zero and alternating lower limbs
    for low in (0, (1 << 224) - 1, sum(0x80000000 << (32 * i) for i in range(7))):
        v += [(t << 224) | low for t in (0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF)]
    v += [0xFFFFFFFF << (32 * i) for i in range(8)] + [ONES ^ (0xFFFFFFFF << (32 * i)) for i in range(8)]
    return v


def quotient_extremes(F, body, n, rng):
    """(tuples with every q_k = 0xFFFFFFFF, tuples with every q_k = 0), about n of each"""
    m = F.m
    odd = lambda: rng.getrandbits(256) | 1
    inv = lambda b: pow(b, -1, R)
    if body == "mul":
        full = [(m, 1), (1, m), (ONES, (-m) % R)]                       # (2^256 - 1) * -m = m (mod 2^256): the largest factor there is
        for _ in range(n):
            b = odd()
            full.append((m * inv(b) % R, b))
        zero = [(0, 0), (0, ONES), (ONES, 0), (1 << 128, 1 << 128), (1 << 255, 2), (ONES << 128 & MASK, ONES << 128 & MASK)]
        for _ in range(n):
            k = rng.randrange(257)
            zero.append(((rng.getrandbits(256) << k) & MASK, (rng.getrandbits(256) << (256 - k)) & MASK))
    elif body == "sqr":
        full = [(r,) for r in sqrt_mod_R(m)]                              # all there are
        zero = [(0,), (1 << 128,), (1 << 255,), (ONES << 128 & MASK,)] + [((rng.getrandbits(128) << 128),) for _ in range(n)]
    else:
        full = [(m, 1, 0, 0), (0, 0, 1, m), (ONES, (-m) % R, 0, ONES), (ONES, ONES, ONES, (1 - m) % R)]     # (-1)(-1) + (-1)(1 - m) = m
        for _ in range(n):
            b, c, d = odd(), rng.getrandbits(256), rng.getrandbits(256)
            full.append(((m - c * d) * inv(b) % R, b, c, d))
        zero = [(0, 0, 0, 0), (ONES, 1, ONES, ONES), (1 << 128, 1 << 128, 1 << 255, 2), (ONES, 0, 0, ONES)]  # -1 + (-1)(-1) = 0
        for _ in range(n):
            b, c, d = odd(), rng.getrandbits(256), rng.getrandbits(256)
            zero.append(((-c * d) * inv(b) % R, b, c, d))
    for t in full:
        assert T_of(body, t) % R == m % R
    for t in zero:
        assert T_of(body, t) % R == 0
    return full, zero


def random_operands(F, body, per_range, rng):
    """per_range tuples each from [0, m), [m, 2m), [2m, 2m + 9 eps) and the uniformly random 256-bit words"""
    m = F.m
    ranges = [(0, m), (m, 2 * m), (2 * m, s.lazy_top(F)), (0, R)]
    return [tuple(rng.randrange(*rg) for _ in range(ARITY[body])) for rg in ranges for _ in range(per_range)]


def adversarial(F, body, n, seed=21):
    """about 3n tuples: the edge operands crossed (as far as n allows), both quotient extremes, and the edges against them"""
    rng = random.Random((seed << 8) | F.fid)
    e = edge_operands(F)
    k = ARITY[body]
    if k == 1:
        cases = [(v,) for v in e]
    elif k == 2:
        cases = [(a, b) for a in e for b in e]
    else:
        cases = [(a, b, a, b) for a in e for b in e] + [(a, a, b, b) for a in e[:24] for b in e[:24]]
    if len(cases) > n:
        cases = cases[:len(e)] + rng.sample(cases[len(e):], n - len(e))
    full, zero = quotient_extremes(F, body, n, rng)
    return cases + full + zero, len(cases), len(full)


def to_limbs(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype="<u4").reshape(len(values), 8)


def from_limbs(cols):
    """8 (or 9) arrays of 32-bit words, least significant first -> Python integers"""
    raw = np.ascontiguousarray(np.stack([np.asarray(c, dtype="<u4") for c in cols], axis=1)).tobytes()
    w = 4 * len(cols)
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def run_model(F, body, tuples, carry_all=False):
    """the emitted schedule on operand tuples -> (the nine-word results as integers, the quotient digits q[0..7] as arrays)"""
    ops = [to_limbs([t[i] for t in tuples]) for i in range(ARITY[body])]
    r, ninth, q = gen.model(gen.schedule(body, carry_all), gen.model_inputs(body, F.name, *ops))
    return from_limbs(r + [ninth]), q


# what the device entry points return for ANY 256-bit operands: the scan keeps eight words (inside every caller's contract
# the ninth is zero), then fe_mul_inl subtracts m once if it can and fe_mul2_lazy subtracts m when bit 255 is set
def dev_mul_lazy(F, a, b):
    return s.redc(F, a * b) & MASK


def dev_sqr_lazy(F, a):
    return s.redc(F, a * a) & MASK


def dev_mul_inl(F, a, b):
    t = s.redc(F, a * b) & MASK
    return t - F.m if t >= F.m else t


def dev_mul2_lazy(F, a, b, c, d):
    t = s.redc(F, a * b + c * d) & MASK
    return t - F.m if t >> 255 else t


DEVICE_OPS = {"fe_mul_inl": ("mul", dev_mul_inl), "fe_mul_lazy": ("mul", dev_mul_lazy), "fe_sqr_lazy": ("sqr", dev_sqr_lazy),
              "fe_mul2_lazy": ("mul2", dev_mul2_lazy)}
