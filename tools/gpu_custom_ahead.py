#!/usr/bin/env python3
"""Measurements of a custom chain's lookahead and early rows (vdf_nova_tuning.custom_ahead) on one MI355X, profiler off (output:
profiles/r20_custom_ahead.txt).  ONE process, t = 2^log2t rounds per step, checkpoints every `--every` rounds, `--steps` steps, W =
`--window`, `--runs` alternating repeats over the same chain of

  custom_ahead = 0 | 1 | 2 | 2 with periodic_rows = 1     circuit F through the seam (tests/custom_chain_spec.py FC)
  the same chain under the built-in forward kind (VDF_CIRCUIT_MINROOT_FORWARD), from the same checkpoints

in the two arrangements of tools/gpu_custom_chain.py, so that its figures from another build are comparable line by line:

  whole     prove_recursively_custom (prove_recursively for the built-in kind): steps / wall time of the WHOLE call, window 0 included
  stepwise  the same loop by hand (materialize / prove_step_custom_chain / release), window 0 waited for and timed apart: the
            steps / wall time of all steps after it

then (--lanes) L = 1, 4, 8 lanes at L * t = 2^log2t (the same rounds per step) for custom_ahead = 0 and 2, `whole` only.  Every
proof is compared byte for byte with custom_ahead = 0's before any time is printed.  --parent FILE: the output of
tools/gpu_custom_chain.py run with the PARENT build's libraries in the same session; its "(c) ... W" and "chain step by step" lines
are the baseline, and a mode is called faster only when its maximum step time is below the parent's minimum."""
import argparse
import os
import re
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
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--lanes", type=int, nargs="*", default=[])
    ap.add_argument("--skip-single", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_custom_ahead.txt"))
    a = ap.parse_args()
    t, every, W = 1 << a.log2t, a.every, a.window
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "a" if a.skip_single else "w")

    def out(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    import numpy as np
    import vdf_amd
    from vdf_amd.minroot import FIELD_FQ, PallasVDF, State
    from vdf_amd.nova import (CIRCUIT_MINROOT_FORWARD, CustomChain, ForwardCircuits, NovaVDFProof, public_params, public_params_custom,
                              record_walk_body)
    from custom_chain_spec import FC
    from custom_lanes_spec import FL
    from walks_spec import minroot_body
    from util import states_array
    med = statistics.median
    out("custom chain, lookahead and early rows: t = 2^%d, checkpoints every %d rounds, %d steps, W = %d, %d alternating repeats; "
        "GPU_MAX_HW_QUEUES = %s" % (a.log2t, every, a.steps, W, a.runs, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    walk_tape = record_walk_body(minroot_body(FIELD_FQ))

    def backwards(seed, intervals, ev, i_last):
        cps = [State.from_ints(FIELD_FQ, 0x123456789ABCDEF + seed, 0xFEDCBA987654321 + 3 * seed, i_last)]
        for _ in range(intervals):
            cps.insert(0, PallasVDF.inverse_eval(cps[0], ev))
        return cps

    def spread(name, rates, parent=None):
        ms = [1e3 / r for r in rates]
        line = "%-58s steps/s: %s  median %.1f, min %.1f, max %.1f | ms per step: median %.3f, min %.3f, max %.3f" % (
            name, " ".join("%.1f" % r for r in rates), med(rates), min(rates), max(rates), med(ms), min(ms), max(ms))
        if parent:
            lo, hi = 1e3 / parent[2], 1e3 / parent[1]                  # the parent's min and max step time
            verdict = "FASTER than the parent (max below its min)" if max(ms) < lo else (
                "SLOWER than the parent (min above its max)" if min(ms) > hi else
                ("inside the parent's min-max" if lo <= med(ms) <= hi else "overlaps the parent's min-max"))
            line += " | parent %.3f .. %.3f ms: %s" % (lo, hi, verdict)
        out(line)

    parent = {}
    if a.parent and os.path.exists(a.parent):
        for ln in open(a.parent):
            m = re.match(r"\(c\) prove_recursively_custom, W = (\d+)\s+steps/s.*?median ([\d.]+), min ([\d.]+), max ([\d.]+)", ln)
            if m and int(m.group(1)) == W:
                parent["whole"] = tuple(float(m.group(k)) for k in (2, 3, 4))
            m = re.match(r"chain step by step, W = (\d+)\s.*steps/s\s+median ([\d.]+), min ([\d.]+), max ([\d.]+)", ln)
            if m and int(m.group(1)) == W:
                parent["stepwise"] = tuple(float(m.group(k)) for k in (2, 3, 4))
        out("parent build, tools/gpu_custom_chain.py in the same session (median, min, max steps/s): whole %s, stepwise %s" % (
            parent.get("whole"), parent.get("stepwise")))

    if not a.skip_single:
        per = t // every
        cps = backwards(0, a.steps * per, every, 7 + a.steps * t)
        arr = states_array(cps)
        xy, i0 = np.ascontiguousarray(arr[:, :8]), np.ascontiguousarray(arr[0, 8:12]).reshape(1, 4)
        z0, zi = [cps[0].x, cps[0].y, cps[0].i], [cps[-1].x, cps[-1].y, cps[-1].i]
        c = FC(t)
        modes = [("custom_ahead = 0", dict(custom_ahead=0)), ("custom_ahead = 1", dict(custom_ahead=1)), ("custom_ahead = 2", dict(custom_ahead=2)),
                 ("custom_ahead = 2, periodic_rows = 1", dict(custom_ahead=2, periodic_rows=1))]
        pps = {name: public_params_custom(ctx, c, **kw) for name, kw in modes}
        for name, _ in modes:
            out("%-38s early rows %s, stencil %d" % (name, pps[name].early_rows(), pps[name].stencil()))
        chain = CustomChain.from_checkpoints(FIELD_FQ, walk_tape, i0, t, every, a.steps, xy.reshape(-1, 4))
        ref, stats = {}, {}

        def same(name, pp, proof):
            assert proof.verify(pp, a.steps, z0, zi) is True, name
            ref.setdefault("bytes", proof.serialize())
            assert proof.serialize() == ref["bytes"], name + ": the proof differs from custom_ahead = 0's"

        def whole(name):
            pp = pps[name]
            ctx.sync()
            t0 = time.perf_counter()
            proof = NovaVDFProof.prove_recursively_custom(pp, c, chain, z0, window_steps=W)
            ctx.sync()
            rate = a.steps / (time.perf_counter() - t0)
            same(name, pp, proof)
            stats[name] = proof.ahead_stats()
            assert chain.memory() == (0, 0)
            proof.free()
            return rate

        def stepwise(name):
            pp, proof = pps[name], None
            ctx.sync()
            chain.materialize(ctx, 0, min(W, a.steps), wait=True)
            t1 = time.perf_counter()
            if W < a.steps:
                chain.materialize(ctx, W, min(W, a.steps - W), wait=False)
            for k in range(a.steps):
                proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
                if (k + 1) % W == 0:
                    chain.release(k + 1 - W, W)
                    b = (k // W + 2) * W
                    if b < a.steps:
                        chain.materialize(ctx, b, min(W, a.steps - b), wait=False)
            ctx.sync()
            rate = a.steps / (time.perf_counter() - t1)
            same("stepwise " + name, pp, proof)
            chain.release()
            proof.free()
            return rate

        # the same chain under the built-in forward kind, from the same checkpoints
        ppf = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)

        def builtin():
            z0f, circuits = ForwardCircuits.begin(t, cps[0])
            for g in range(a.steps):
                circuits.push_checkpoints(every, cps[g * per:g * per + per + 1])
            ctx.sync()
            t0 = time.perf_counter()
            proof = NovaVDFProof.prove_recursively(ppf, circuits, t, z0f, window_steps=W)
            ctx.sync()
            rate = a.steps / (time.perf_counter() - t0)
            assert proof.verify(ppf, a.steps, z0f, zi) is True
            proof.free(); circuits.free()
            return rate

        jobs = [("whole     " + n, lambda n=n: whole(n)) for n, _ in modes] + [("stepwise  " + n, lambda n=n: stepwise(n)) for n, _ in modes] + \
               [("whole     built-in forward kind (prove_recursively)", builtin)]
        rates = {n: [] for n, _ in jobs}
        for _, fn in jobs:                                         # once untimed: allocations, tables, the side queues; and every proof compared
            fn()
        for _ in range(a.runs):
            for n, fn in jobs:
                rates[n].append(fn())
        for n, _ in jobs:
            spread(n, rates[n], parent.get(n.split()[0]) if "custom_ahead" in n else None)
        for name, _ in modes:
            out("%-38s (hits, misses, skipped) of the %d steps after the first: %s" % (name, a.steps - 1, stats[name]))
        chain.free()
        ppf.free()
        for pp in pps.values():
            pp.free()

    for L in a.lanes:
        tl = t // L
        ev = min(every, tl)
        per = tl // ev
        lanes_cps = [backwards(l, a.steps * per, ev, 7 + 1000 * l + a.steps * tl) for l in range(L)]
        arr = np.concatenate([np.ascontiguousarray(states_array(x)[:, :8]).reshape(-1, 4) for x in lanes_cps])
        inv = np.concatenate([np.ascontiguousarray(states_array(x)[0, 8:12]).reshape(1, 4) for x in lanes_cps])
        z0 = [v for x in lanes_cps for v in (x[0].x, x[0].y, x[0].i)]
        zi = [v for x in lanes_cps for v in (x[-1].x, x[-1].y, x[-1].i)]
        chain = CustomChain.lanes_from_checkpoints(FIELD_FQ, walk_tape, inv, tl, ev, a.steps, L, arr)
        c = FL(tl, L)
        pps = {m: public_params_custom(ctx, c, custom_ahead=m) for m in (0, 2)}
        ref, stats = {}, {}

        def prove(m):
            ctx.sync()
            t0 = time.perf_counter()
            proof = NovaVDFProof.prove_recursively_custom(pps[m], c, chain, z0, window_steps=W)
            ctx.sync()
            rate = a.steps / (time.perf_counter() - t0)
            assert proof.verify(pps[m], a.steps, z0, zi) is True
            ref.setdefault("bytes", proof.serialize())
            assert proof.serialize() == ref["bytes"], "lanes: the proof differs from custom_ahead = 0's"
            stats[m] = proof.ahead_stats()
            proof.free()
            return rate
        rates = {0: [], 2: []}
        for m in (0, 2):
            prove(m)
        for _ in range(a.runs):
            for m in (0, 2):
                rates[m].append(prove(m))
        for m in (0, 2):
            spread("whole     L = %d lanes of t = %d, custom_ahead = %d %s" % (L, tl, m, stats[m]), rates[m])
        chain.free()
        for pp in pps.values():
            pp.free()
    ctx.close()


if __name__ == "__main__":
    main()
