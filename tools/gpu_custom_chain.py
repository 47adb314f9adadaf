#!/usr/bin/env python3
"""Measurements of a custom circuit's chain (vdf_custom_chain, vdf_nova_prove_recursively_custom) on one MI355X, profiler off
(output: profiles/r17_custom_chain.txt).  ONE process, t = 2^log2t rounds per step, checkpoints every `--every` rounds, `--steps`
steps, `--runs` alternating repeats of four arrangements over the same chain and the same parameters:

  (a) one walk launch per step on the prover's own queue, then prove_step_custom      (tools/gpu_custom_walk.py, way "walk")
  (b) a ready host trace uploaded per step, then prove_step_custom                    (tools/gpu_custom_walk.py, way "upload")
  (c) prove_recursively_custom at every `--windows` length: the walks of a window on a side queue, a window ahead
  (d) the same with VDF_CUSTOM_CHECK_STEPS: every step's fresh instance scanned (one sparse product and k_unsat_rows)

Every rate is steps / wall time of the WHOLE chain (for (c) and (d) that includes window 0, which is waited for); (a) and (b) are
also given over the steps after `--warmup`, as profiles/r14_custom_walk.txt gives them.  The yardstick of (c) is (b) in the same
run.  Then the chain driven step by step with window 0 timed apart, and where a step's time goes, by vdf_nova_last_step_ms: the median over the steps of (b) and of the chain driven step by
step (materialize / prove_step_custom_chain / release, the loop prove_recursively_custom runs)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=16)
    ap.add_argument("--every", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--windows", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_custom_chain.txt"))
    a = ap.parse_args()
    t, every = 1 << a.log2t, a.every
    per = t // every
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "w")

    def out(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    import numpy as np
    import torch
    import vdf_amd
    from vdf_amd._lib import lib
    from vdf_amd.minroot import FIELD_FQ, PallasVDF, State
    from vdf_amd.nova import CustomChain, NovaVDFProof, public_params_custom, record_walk_body, walk_tape_eval
    from custom_chain_spec import FC
    from walks_spec import minroot_body
    from util import dev, states_array
    out("custom chain, t = 2^%d, %d walks of %d rounds per step, %d steps, %d repeats; GPU_MAX_HW_QUEUES = %s" % (
        a.log2t, per, every, a.steps, a.runs, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    # the chain, backwards from an arbitrary last state (the inverse round is cheap): one checkpoint per interval
    cps = [State.from_ints(FIELD_FQ, 0x123456789ABCDEF, 0xFEDCBA987654321, 7 + a.steps * t)]
    for _ in range(a.steps * per):
        cps.insert(0, PallasVDF.inverse_eval(cps[0], every))
    arr = states_array(cps)
    xy, i0 = np.ascontiguousarray(arr[:, :8]), np.ascontiguousarray(arr[0, 8:12]).reshape(1, 4)
    z0, zi = [cps[0].x, cps[0].y, cps[0].i], [cps[-1].x, cps[-1].y, cps[-1].i]
    walk_tape = record_walk_body(minroot_body(FIELD_FQ))
    d_starts = [dev(xy[g * per + 1:g * per + per + 1]) for g in range(a.steps)]
    d_expect = [dev(xy[g * per:g * per + per]) for g in range(a.steps)]
    d_trace = torch.zeros((2 * (t + 1), 4), dtype=torch.int64, device="cuda")
    d_ok = torch.zeros(per, dtype=torch.int32, device="cuda")
    host_traces = []
    for g in range(a.steps):                                    # the traces of (b), by the host evaluator of the same tape
        e, buf = xy[g * per + 1:g * per + per + 1].reshape(-1, 4).copy(), np.zeros((2 * (t + 1), 4), dtype="<u8")
        walk_tape_eval(FIELD_FQ, walk_tape, i0, e, per, every, buf, walk_stride=every, top=every, group=per, group_stride=t + 1, j_base=g * t,
                       heads=True)
        host_traces.append(buf)
    c = FC(t)
    pp = public_params_custom(ctx, c)
    chain = CustomChain.from_checkpoints(FIELD_FQ, walk_tape, i0, t, every, a.steps, xy.reshape(-1, 4))
    out("chain: %d bytes on the host; a window of W steps holds W x %d bytes of traces" % (chain.host_bytes(), (t + 1) * 64))
    reference = {}

    def same_proof(name, proof):
        assert proof.verify(pp, a.steps, z0, zi) is True, name
        reference.setdefault("bytes", proof.serialize())
        assert proof.serialize() == reference["bytes"], name + ": the proof differs from the first arrangement's"

    def per_step(way, ms=None):
        proof, t0, t_all = None, None, time.perf_counter()
        for g in range(a.steps):
            if g == a.warmup:
                ctx.sync()
                t0 = time.perf_counter()
            if way == "a":
                st = d_starts[g].clone()
                ctx.round_tape_walk(FIELD_FQ, walk_tape, i0, st, per, every, d_trace, walk_stride=every, top=every, group=per,
                                    group_stride=t + 1, j_base=g * t, heads=True, expect=d_expect[g], ok=d_ok)
            else:
                assert lib.vdf_dev_memcpy(ctx.handle, d_trace.data_ptr(), host_traces[g].ctypes.data, host_traces[g].nbytes) == 0
            c.advice = d_trace
            proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
            if ms is not None and g >= a.warmup:
                ms.append(proof.last_step_ms())
        ctx.sync()
        now = time.perf_counter()
        c.advice = None
        same_proof(way, proof)
        proof.free()
        return a.steps / (now - t_all), (a.steps - a.warmup) / (now - t0)

    def whole(W, check):
        ctx.sync()
        t0 = time.perf_counter()
        proof = NovaVDFProof.prove_recursively_custom(pp, c, chain, z0, window_steps=W, check_steps=check)
        ctx.sync()
        rate = a.steps / (time.perf_counter() - t0)
        same_proof("W = %d" % W, proof)
        assert chain.memory() == (0, 0)
        proof.free()
        return rate

    def stepwise_chain(W, ms):
        """the loop of prove_recursively_custom by hand, for the per-step times"""
        proof = None
        ctx.sync()
        t0 = time.perf_counter()
        chain.materialize(ctx, 0, min(W, a.steps), wait=True)
        t1 = time.perf_counter()
        if W < a.steps:
            chain.materialize(ctx, W, min(W, a.steps - W), wait=False)
        for k in range(a.steps):
            proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
            if k >= a.warmup:
                ms.append(proof.last_step_ms())
            if (k + 1) % W == 0:
                chain.release(k + 1 - W, W)
                b = (k // W + 2) * W
                if b < a.steps:
                    chain.materialize(ctx, b, min(W, a.steps - b), wait=False)
        ctx.sync()
        t2 = time.perf_counter()
        same_proof("stepwise W = %d" % W, proof)
        chain.release()
        proof.free()
        return 1e3 * (t1 - t0), a.steps / (t2 - t1)

    arrangements = [("(a) one walk launch per step, the prover's queue", lambda: per_step("a")),
                    ("(b) a host trace uploaded per step", lambda: per_step("b"))]
    for W in a.windows:
        arrangements.append(("(c) prove_recursively_custom, W = %d" % W, lambda W=W: (whole(W, False), None)))
    for W in a.windows:
        arrangements.append(("(d) ... with VDF_CUSTOM_CHECK_STEPS, W = %d" % W, lambda W=W: (whole(W, True), None)))
    rates = {name: [] for name, _ in arrangements}
    for name, fn in arrangements:                               # once untimed: allocations, tables, the side queue
        fn()
    for _ in range(a.runs):
        for name, fn in arrangements:
            rates[name].append(fn())
    med = {}
    for name, _ in arrangements:
        r = [x[0] for x in rates[name]]
        med[name] = (statistics.median(r), min(r), max(r))
        line = "%-50s steps/s over all %d steps: %s  median %.1f, min %.1f, max %.1f" % (name, a.steps, " ".join("%.1f" % x for x in r), *med[name])
        if rates[name][0][1] is not None:
            w = [x[1] for x in rates[name]]
            line += "; after %d steps: median %.1f, min %.1f, max %.1f" % (a.warmup, statistics.median(w), min(w), max(w))
        out(line)
    b = med[arrangements[1][0]]
    for name, _ in arrangements[2:]:
        m = med[name][0]
        verdict = "inside (b)'s spread" if b[1] <= m <= b[2] else ("above (b)'s maximum" if m > b[2] else "BELOW (b)'s minimum")
        out("%-50s median / (b)'s median = %.3f: %s [%.1f, %.1f]" % (name, m / b[0], verdict, b[1], b[2]))
    # where a step's time goes
    # the same loop by hand, window 0 timed apart: what nothing hides, and the rate once the walks run a window ahead
    for W in a.windows:
        runs = [stepwise_chain(W, []) for _ in range(a.runs)]
        w0, r = [x[0] for x in runs], [x[1] for x in runs]
        out("chain step by step, W = %-2d  window 0 (materialize, waited for): median %.1f ms, min %.1f, max %.1f; all %d steps after it: %s steps/s  "
            "median %.1f, min %.1f, max %.1f" % (W, statistics.median(w0), min(w0), max(w0), a.steps, " ".join("%.1f" % x for x in r),
                                                 statistics.median(r), min(r), max(r)))
    ms_b, ms_c = [], []
    per_step("b", ms_b)
    stepwise_chain(a.windows[0], ms_c)
    keys = list(ms_b[0].keys()) if isinstance(ms_b[0], dict) else list(range(len(ms_b[0])))
    get = (lambda d, k: d[k])
    out("median ms per step phase (vdf_nova_last_step_ms) over the steps after %d:" % a.warmup)
    out("  %-28s %s" % ("phase", "  ".join("%10s" % str(k)[:10] for k in keys)))
    for label, rows in (("(b) uploaded trace", ms_b), ("chain step by step, W = %d" % a.windows[0], ms_c)):
        out("  %-28s %s" % (label, "  ".join("%10.3f" % statistics.median(get(r, k) for r in rows) for k in keys)))
    chain.free()
    pp.free()
    ctx.close()


if __name__ == "__main__":
    main()
