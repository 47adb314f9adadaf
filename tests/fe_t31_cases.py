"""Operand lists for the bounded-top column scans (vdf_amd/csrc/fe_{mul,sqr,mul2}_t31_gfx950.inc: limb 7 of every multiplicand at
most 0x80000000), the bridge to the integer model of their emitted schedule (tools/gen_fe_mul.py: schedule(top31=True)), and a
job-file writer for their op ids in tools/ubench/prim_check.  Shared by tests/test_fe_t31_model.py (no device) and
tests/test_gpu_fe_t31.py.  Every list here is INSIDE the precondition; the lists that leave it on purpose are
tests/fe_scan_cases.py's, for the generic bodies."""
import os
import struct
import subprocess
import tempfile

import fe_scan_cases as c
import prim_spec as s

gen = c.gen
R, MASK = s.R, s.MASK
TOP = 1 << 31                                # the largest limb 7 the bodies were generated for
# name -> (op id, words in, words out, body, eight-word semantics): tools/ubench/prim_check.hip
T31_OPS = {"fe_mul_lazy_t31": (31, 2, 1, "mul", c.dev_mul_lazy), "fe_sqr_lazy_t31": (32, 1, 1, "sqr", c.dev_sqr_lazy),
           "fe_mul2_lazy_t31": (33, 4, 1, "mul2", c.dev_mul2_lazy)}


def bounded(v):
    return 0 <= v < R and (v >> 224) <= TOP


def rand_bounded(rng):
    """uniform over the 256-bit words with limb 7 <= 2^31"""
    return rng.randrange((TOP + 1) << 224)


def random_operands(F, body, per_range, rng):
    """per_range tuples each from [0, m), [m, 2m), [2m, 2m + 9 eps) and the uniformly random words with limb 7 <= 2^31"""
    m = F.m
    out = [tuple(rng.randrange(*rg) for _ in range(c.ARITY[body])) for rg in ((0, m), (m, 2 * m), (2 * m, s.lazy_top(F))) for _ in range(per_range)]
    return out + [tuple(rand_bounded(rng) for _ in range(c.ARITY[body])) for _ in range(per_range)]


def edge_operands(F):
    """those of fe_scan_cases.edge_operands inside the precondition -- among them limb 7 = 0x80000000 over all-ones lower
    limbs, the largest operand the bodies accept (outside the lazy contract, inside the precondition)"""
    e = [v for v in c.edge_operands(F) if bounded(v)]
    assert (TOP << 224) | ((1 << 224) - 1) in e and 1 << 255 in e and s.lazy_top(F) in e
    return e


def quotient_extremes(F, body, n, rng):
    """(tuples with every q_k = 0xFFFFFFFF, tuples with every q_k = 0), all factors with limb 7 <= 2^31.  T = m (mod 2^256):
    draw the other factors bounded (b odd) and keep the tuple when the factor solved for is bounded too -- about half are"""
    m = F.m
    inv = lambda b: pow(b, -1, R)

    def solve(target):
        while True:
            if body == "mul":
                b = rand_bounded(rng) | 1
                t = (target * inv(b) % R, b)
            else:
                b, cc, d = rand_bounded(rng) | 1, rand_bounded(rng), rand_bounded(rng)
                t = ((target - cc * d) * inv(b) % R, b, cc, d)
            if bounded(t[0]):
                return t

    if body == "sqr":
        full = [(r,) for r in c.sqrt_mod_R(m) if r < 1 << 255]          # the square roots of m below 2^255
        zero = [(0,), (1 << 128,), (1 << 255,), ((1 << 255) - (1 << 128),)] + [(rng.getrandbits(127) << 128,) for _ in range(n)]
    else:
        full = [(m, 1), (1, m)] if body == "mul" else [(m, 1, 0, 0), (0, 0, 1, m)]
        full += [solve(m) for _ in range(n)]
        if body == "mul":
            zero = [(0, 0), (0, (TOP << 224) | ((1 << 224) - 1)), (1 << 128, 1 << 128), (1 << 255, 2), (1 << 255, 1 << 255)]
            while len(zero) < n + 5:
                k = rng.randrange(257)
                t = ((rng.getrandbits(256) << k) & MASK, (rng.getrandbits(256) << (256 - k)) & MASK)
                if all(map(bounded, t)):
                    zero.append(t)
        else:
            zero = [(0, 0, 0, 0), (1 << 128, 1 << 128, 1 << 255, 2), (1 << 255, 1 << 255, 1 << 255, 1 << 255)]
            zero += [solve(0) for _ in range(n)]
    for t in full:
        assert c.T_of(body, t) % R == m % R and all(map(bounded, t))
    for t in zero:
        assert c.T_of(body, t) % R == 0 and all(map(bounded, t))
    return full, zero


def adversarial(F, body, n, seed=31):
    """the bounded edge operands crossed (as far as n allows), then both quotient extremes: (tuples, edge count, full count)"""
    import random
    rng = random.Random((seed << 8) | F.fid)
    e = edge_operands(F)
    k = c.ARITY[body]
    if k == 1:
        cases = [(v,) for v in e]
    elif k == 2:
        cases = [(a, b) for a in e for b in e]
    else:
        cases = [(a, b, a, b) for a in e for b in e] + [(a, a, b, b) for a in e for b in e]
    if len(cases) > n:
        cases = cases[:len(e)] + rng.sample(cases[len(e):], n - len(e))
    full, zero = quotient_extremes(F, body, n, rng)
    return cases + full + zero, len(cases), len(full)


def run_model(F, body, tuples):
    """the emitted bounded-top schedule on operand tuples -> (the nine-word results as integers, the quotient digits)"""
    ops = [c.to_limbs([t[i] for t in tuples]) for i in range(c.ARITY[body])]
    r, ninth, q = gen.model(gen.schedule(body, top31=True), gen.model_inputs(body, F.name, *ops))
    return c.from_limbs(r + [ninth]), q


def run_jobs(jobs, timeout=120):
    """jobs: [(field, name in T31_OPS, rows of integers)] -> [rows of one-word tuples], through ONE child process on the device"""
    assert os.path.exists(s.PRIM_CHECK), "tools/ubench/prim_check is not built: make -C vdf_amd/csrc"
    blob = [b"PRIMJOB1", struct.pack("<I", len(jobs))]
    for F, op, rows in jobs:
        oid, nin = T31_OPS[op][:2]
        assert all(len(r) == nin and all(map(bounded, r)) for r in rows), op
        blob.append(struct.pack("<4I", F.fid, oid, len(rows), nin))
        blob.append(b"".join(int(v).to_bytes(32, "little") for r in rows for v in r))
    with tempfile.TemporaryDirectory() as d:
        jf, rf = os.path.join(d, "jobs.bin"), os.path.join(d, "results.bin")
        with open(jf, "wb") as f:
            f.write(b"".join(blob))
        r = subprocess.run([s.PRIM_CHECK, jf, rf], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, "prim_check exit %d: %s%s" % (r.returncode, r.stdout, r.stderr)
        with open(rf, "rb") as f:
            data = f.read()
    assert data[:8] == b"PRIMOUT1" and struct.unpack_from("<I", data, 8)[0] == len(jobs)
    pos, res = 12, []
    for F, op, rows in jobs:
        oid, _, nout = T31_OPS[op][:3]
        assert struct.unpack_from("<4I", data, pos) == (F.fid, oid, len(rows), nout)
        pos += 16
        res.append([(int.from_bytes(data[pos + 32 * i: pos + 32 * i + 32], "little"),) for i in range(len(rows))])
        pos += 32 * len(rows)
    assert pos == len(data)
    return res
