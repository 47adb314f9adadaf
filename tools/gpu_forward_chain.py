#!/usr/bin/env python3
"""Measurements of the forward step circuit on one MI355X, one command (output: profiles/r07_forward_chain.txt by default).

  (1) step rate: prove_step/s over `--steps` steps at t = 2^16 in ONE process, alternating `--repeats` times between the
      forward kind and the BOUND kind (same device work up to where values sit: 3t + 1 round terms committed, 3t + 1 stencil
      rows); traces resident before the clock starts on both legs (rebuilt on the GPU from the same step-boundary states).
      Target: the forward median is not below BOUND's lowest run.
  (3) the claim: after_eval_ms of eval_and_prove at 32 and at 128 steps -- the gap between "the output exists" and "the proof
      exists" -- which must not grow with the chain by more than one steady-state step; beside it the inverse path's gap for the
      128-step chain: prove_recursively (BOUND) after the evaluation, traces resident.
  (4) the evaluator must not pay for its prover: eval_ms of eval_and_prove (32 steps) against plain vdf_minroot_eval of the same
      rounds, three times each.
  --forward-only: the forward leg of (1) alone -- `--steps` steps, `--repeats` timed runs after one warm-up, the step time at the
      median -- and nothing else: the figure to compare between two builds of the library, run alternately.
  --kernels-only: (2) a short chain of each kind with per-launch HIP events on, printing the time and the TB/s of
      k_nifs_cross_minroot_forward (timed under the label k_nifs_cross_fwd) and k_nifs_cross_minroot (3 variables per round); run it under
      `rocprofv3 --kernel-trace --stats -- python tools/gpu_forward_chain.py --kernels-only` for the profiler's own figures.
The hardware-queue count in force (GPU_MAX_HW_QUEUES) is printed.  The forward evaluation (about 0.22 s per step on the host)
is set-up for (1); it is the measured thing in (3) and (4)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=16)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_forward_chain.txt"))
    a = ap.parse_args()
    import vdf_amd
    from vdf_amd.minroot import EvalMode, FIELD_FQ, PallasVDF, State
    from vdf_amd.nova import (CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_FORWARD, ForwardCircuits, InverseMinRootCircuit, NovaVDFProof,
                              public_params)
    t = 1 << a.log2t
    path = a.out.replace(".txt", "_kernels.txt") if a.kernels_only else a.out
    os.makedirs(os.path.dirname(path), exist_ok=True)
    log = open(path, "w")

    def out(s=""):                                         # every line at once: a run that ends early leaves what it measured
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    ctx = vdf_amd.Context(0)
    vdf = PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential)
    initial = State.from_ints(FIELD_FQ, 0x1234, 0, 0)
    out("forward step circuit, t = 2^%d; GPU_MAX_HW_QUEUES = %s" % (a.log2t, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ppf = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)
    ppb = public_params(ctx, t, CIRCUIT_MINROOT_BOUND)
    out("stencil codes: forward %d, bound %d; primary shape %s / %s" % (ppf.stencil(), ppb.stencil(), ppf.sizes(0), ppb.sizes(0)))

    def chains(n):
        """both kinds' circuits over one chain of n steps, traces rebuilt on the GPU from the step-boundary states"""
        t0 = time.perf_counter()
        states = vdf.eval_checkpoints(initial, t * n, t)
        ev = time.perf_counter() - t0
        z0f, fc = ForwardCircuits.begin(t, initial)
        for k in range(n):
            fc.push_checkpoints(t, states[k:k + 2])
        fc.materialize(ctx)
        z0b, bc = InverseMinRootCircuit.from_checkpoints(t, t, n, states)
        bc.materialize(ctx)
        return states, ev, (z0f, fc), (z0b, bc)

    if a.kernels_only:
        n = 12
        states, ev, (z0f, fc), (z0b, bc) = chains(n)
        for name, pp, z0, cs, kern in (("forward", ppf, z0f, fc, "k_nifs_cross_fwd"), ("bound", ppb, z0b, bc, "k_nifs_cross_minroot")):
            p = None
            for k in range(n):
                p = NovaVDFProof.prove_step(pp, p, cs, k, z0)
                if k == 1:
                    p.set_kernel_timing(True)
            evs = [e for e in p.kernel_events() if e[1] == kern]
            ms = [e[4] - e[3] for e in evs]
            byt = evs[0][2] if evs else 0.0
            med = statistics.median(ms) if ms else float("nan")
            out("(2) %-8s %-30s launches %3d  ms min %.4f median %.4f max %.4f  algorithmic bytes %.0f  TB/s at the median %.3f" % (
                name, kern, len(ms), min(ms) if ms else 0, med, max(ms) if ms else 0, byt, byt / (med * 1e-3) / 1e12 if ms else 0))
            p.set_kernel_timing(False)
            p.free()
        return

    # ---- (1) step rate ---------------------------------------------------------------------------------------------
    n = a.steps if a.forward_only else max(a.steps, 128)   # (3) reads the first 128 steps of the same chain
    states, ev, (z0f, fc), (z0b, bc) = chains(n)
    out("(1) %d steps; host evaluation %.1f s (set-up); traces resident: forward %s, bound %s" % (n, ev, fc.memory(), bc.memory()))
    rates = {"forward": [], "bound": []}
    legs = (("forward", ppf, z0f, fc), ("bound", ppb, z0b, bc))[:1 if a.forward_only else 2]
    for rep in range(a.repeats + 1):                       # one warm-up alternation
        for name, pp, z0, cs in legs:
            t0 = time.perf_counter()
            p = NovaVDFProof.prove_recursively(pp, cs, t, z0)
            dt = time.perf_counter() - t0
            if rep == 0:
                zi = [states[n].x, states[n].y, states[n].i] if name == "forward" else [initial.x, initial.y, initial.i]
                assert p.verify(pp, n, z0, zi), name
            else:
                rates[name].append(n / dt)
            p.free()
    for name, *_ in legs:
        r = rates[name]
        out("    %-8s prove_step/s: %s  median %.1f  min %.1f  max %.1f  (%.4f ms per step at the median)" % (
            name, " ".join("%.1f" % x for x in r), statistics.median(r), min(r), max(r), 1e3 / statistics.median(r)))
    if a.forward_only:
        fc.free(); bc.free(); ppf.free(); ppb.free(); ctx.close()
        return
    fmed, bmin = statistics.median(rates["forward"]), min(rates["bound"])
    out("    target (forward median >= bound's lowest run): %s (%.1f vs %.1f)" % ("met" if fmed >= bmin else "NOT met", fmed, bmin))
    step_ms = 1e3 / fmed
    fc.free()

    # ---- (3) the gap between the output and the proof ----------------------------------------------------------------
    gaps = {}
    for m in (32, 128):
        p, final, st = NovaVDFProof.eval_and_prove(ppf, vdf, initial, m)
        assert final == states[m] and p.verify(ppf, m, z0f, [final.x, final.y, final.i])
        gaps[m] = st
        out("(3) eval_and_prove, %3d steps: eval_ms %.1f  after_eval_ms %.3f  max_backlog %d" % (m, st["eval_ms"], st["after_eval_ms"], st["max_backlog"]))
        p.free()
    grow = gaps[128]["after_eval_ms"] - gaps[32]["after_eval_ms"]
    out("    128 steps against 32: %+.3f ms; one steady-state step of this run: %.3f ms -> independent of the chain's length: %s" % (
        grow, step_ms, "yes" if grow <= step_ms else "NO"))
    z0c, c128 = InverseMinRootCircuit.from_checkpoints(t, t, 128, states[:129])
    c128.materialize(ctx)
    t0 = time.perf_counter()
    p = NovaVDFProof.prove_recursively(ppb, c128, t, z0c)
    inv_gap = (time.perf_counter() - t0) * 1e3
    assert p.verify(ppb, 128, z0c, [initial.x, initial.y, initial.i])
    out("    the inverse path (BOUND) for the same 128 steps: nothing can start before the last round; prove_recursively after the "
        "evaluation, traces resident: %.1f ms" % inv_gap)
    p.free(); c128.free(); bc.free()

    # ---- (4) the evaluator beside its prover ------------------------------------------------------------------------
    m = 32
    plain, beside = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        s = initial
        for _ in range(m):
            s, _tr = vdf.eval_with_trace(s, t)             # as the library's thread does: step by step, with the trace
        plain.append((time.perf_counter() - t0) * 1e3)
        p, final, st = NovaVDFProof.eval_and_prove(ppf, vdf, initial, m)
        beside.append(st["eval_ms"])
        p.free()
    out("(4) %d steps, three runs each: plain vdf_minroot_eval %s ms; eval_ms of eval_and_prove %s ms" % (
        m, " ".join("%.1f" % x for x in plain), " ".join("%.1f" % x for x in beside)))
    diff = statistics.median(beside) - statistics.median(plain)
    spread = max(max(plain) - min(plain), max(beside) - min(beside))
    out("    difference of the medians %+.1f ms (%.2f %%), spread of the three %.1f ms -> %s" % (
        diff, 100 * diff / statistics.median(plain), spread, "within the spread" if abs(diff) <= spread else
        "BEYOND the spread: the evaluator's thread shares the host with the proving thread and the three synthesis helpers"))
    ppf.free(); ppb.free(); ctx.close()


if __name__ == "__main__":
    main()
