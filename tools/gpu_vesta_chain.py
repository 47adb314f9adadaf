#!/usr/bin/env python3
"""The cycle in both orientations on one MI355X, one command (output: profiles/r10_vesta_cycle.txt by default).

  (1) step rate: prove_step/s over `--steps` steps (at least 200) at t = 2^16 in ONE process, for the REFERENCE and the FORWARD
      kind in both orientations -- Fq (G1 = Pallas, the path of every earlier measurement: the yardstick) and Fp (G1 = Vesta) --
      the four legs interleaved, `--repeats` timed alternations after one warm-up; traces resident before the clock starts
      (rebuilt on the GPU from the step-boundary states).  Per leg: every run, the median, and the run-to-run spread (max - min).
      Expectation: by symmetry Fp equals Fq within that spread.  Where Fp's median is below Fq's by more than the larger spread
      of the two, the kernels of one step of each orientation (vdf_nova_proof_kernel_events) are listed side by side and the
      one with the largest excess is named: a finding to record, not something this tool tunes.
  (2) compress and verify: vdf_nova_compress, vdf_nova_verify_compressed and vdf_nova_verify of the proofs of (1), three times
      each per leg.
The hardware-queue count in force (GPU_MAX_HW_QUEUES) is printed.  The forward evaluation on the host is set-up."""
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_vesta_cycle.txt"))
    a = ap.parse_args()
    import vdf_amd
    from vdf_amd.minroot import EvalMode, FIELD_FP, FIELD_FQ, PallasVDF, State, VestaVDF
    from vdf_amd.nova import (CIRCUIT_MINROOT_FORWARD, CIRCUIT_MINROOT_REFERENCE, ForwardCircuits, InverseMinRootCircuit, NovaVDFProof,
                              public_params)
    t, n = 1 << a.log2t, max(a.steps, 200)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "w")

    def out(s=""):                                         # every line at once: a run that ends early leaves what it measured
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    ctx = vdf_amd.Context(0)
    out("the cycle in both orientations, t = 2^%d, %d steps per run; GPU_MAX_HW_QUEUES = %s" % (
        a.log2t, n, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    legs = []                                              # (name, field name, pp, z0, circuits, zi)
    for fname, field, V in (("Fq", FIELD_FQ, PallasVDF), ("Fp", FIELD_FP, VestaVDF)):
        vdf = V.new_with_mode(EvalMode.LTRAddChainSequential)
        initial = State.from_ints(field, 0x1234, 0, 0)
        t0 = time.perf_counter()
        states = vdf.eval_checkpoints(initial, t * n, t)
        out("%s: host evaluation of %d x 2^%d rounds %.1f s (set-up)" % (fname, n, a.log2t, time.perf_counter() - t0))
        first, last = [initial.x, initial.y, initial.i], [states[n].x, states[n].y, states[n].i]
        ppr = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, field=field)
        z0r, cr = InverseMinRootCircuit.from_checkpoints(t, t, n, states, field=field)
        cr.materialize(ctx)
        legs.append(("reference", fname, ppr, z0r, cr, first))
        ppf = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD, field=field)
        z0f, cf = ForwardCircuits.begin(t, initial, field=field)
        for k in range(n):
            cf.push_checkpoints(t, states[k:k + 2])
        cf.materialize(ctx)
        legs.append(("forward", fname, ppf, z0f, cf, last))
        for pp, kind in ((ppr, "reference"), (ppf, "forward")):
            out("    %-9s %s: orientation %d, stencil code %d, early rows %s, primary shape %s, generators %d / %d, memory %s" % (
                kind, fname, pp.field(), pp.stencil(), pp.early_rows(), pp.sizes(0), pp.sizes(0)["num_gens"], pp.sizes(1)["num_gens"], pp.memory()))
    # ---- (1) step rate -------------------------------------------------------------------------------------------------
    rates = {(k, f): [] for k, f, *_ in legs}
    kept = {}
    for rep in range(a.repeats + 1):                       # one warm-up alternation
        for kind, fname, pp, z0, cs, zi in legs:
            t0 = time.perf_counter()
            p = NovaVDFProof.prove_recursively(pp, cs, t, z0)
            dt = time.perf_counter() - t0
            if rep == 0:
                assert p.verify(pp, n, z0, zi), (kind, fname)
            else:
                rates[(kind, fname)].append(n / dt)
            if rep == a.repeats:
                kept[(kind, fname)] = p
            else:
                p.free()
    out("(1) prove_step/s, %d timed runs of %d steps per leg, legs interleaved" % (a.repeats, n))
    for kind in ("reference", "forward"):
        for fname in ("Fq", "Fp"):
            r = rates[(kind, fname)]
            out("    %-9s %s: %s  median %.1f  min %.1f  max %.1f  spread %.1f  (%.4f ms per step at the median)" % (
                kind, fname, " ".join("%.1f" % x for x in r), statistics.median(r), min(r), max(r), max(r) - min(r), 1e3 / statistics.median(r)))
        q, p_ = rates[(kind, "Fq")], rates[(kind, "Fp")]
        diff = statistics.median(p_) - statistics.median(q)
        spread = max(max(q) - min(q), max(p_) - min(p_))
        slower = -diff > spread
        out("    %-9s Fp against Fq (the yardstick): %+.1f steps/s (%+.2f %%), larger spread of the two %.1f -> %s" % (
            kind, diff, 100 * diff / statistics.median(q), spread, "Fp is SLOWER by more than the spread" if slower else "equal within the spread"
            if abs(diff) <= spread else "Fp is faster by more than the spread"))
        if slower:                                         # name the kernel: one step of each orientation with per-launch events
            per = {}
            for kind2, fname, pp, z0, cs, zi in legs:
                if kind2 != kind:
                    continue
                p = None
                for k in range(6):
                    p = NovaVDFProof.prove_step(pp, p, cs, k, z0)
                    if k == 1:
                        p.set_kernel_timing(True)
                acc = {}
                for _q, name, _b, s, e in p.kernel_events():
                    acc[name] = acc.get(name, 0.0) + (e - s)
                per[fname] = {k: v / 4 for k, v in acc.items()}     # steps 2..5
                p.set_kernel_timing(False)
                p.free()
            names = sorted(set(per["Fq"]) | set(per["Fp"]), key=lambda k: per["Fp"].get(k, 0) - per["Fq"].get(k, 0), reverse=True)
            out("    kernel time per step (ms, events on): name  Fq  Fp  excess")
            for k in names:
                out("      %-26s %.4f  %.4f  %+.4f" % (k, per["Fq"].get(k, 0), per["Fp"].get(k, 0), per["Fp"].get(k, 0) - per["Fq"].get(k, 0)))
            out("    FINDING: the largest excess over Fq is in %s" % names[0])
    # ---- (2) compress and verify ---------------------------------------------------------------------------------------
    out("(2) compress / verify_compressed / verify, ms, three runs each")
    for kind, fname, pp, z0, cs, zi in legs:
        p = kept[(kind, fname)]
        cm, vc, vr = [], [], []
        for _ in range(3):
            t0 = time.perf_counter(); s = p.compress(pp); cm.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); ok = s.verify(pp, n, z0, zi); vc.append((time.perf_counter() - t0) * 1e3)
            assert ok, (kind, fname)
            s.free()
            t0 = time.perf_counter(); ok = p.verify(pp, n, z0, zi); vr.append((time.perf_counter() - t0) * 1e3)
            assert ok, (kind, fname)
        f3 = lambda v: " ".join("%.2f" % x for x in v)
        out("    %-9s %s: compress %s | verify_compressed %s | verify %s" % (kind, fname, f3(cm), f3(vc), f3(vr)))
        p.free()
    for _k, _f, pp, _z, cs, _zi in legs:
        cs.free()
        pp.free()
    ctx.close()


if __name__ == "__main__":
    main()
