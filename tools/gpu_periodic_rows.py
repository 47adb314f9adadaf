#!/usr/bin/env python3
"""Measurements of the periodic rows of a custom circuit (vdf_nifs_cross_term_periodic) on one MI355X, profiler off, in ONE process
(output: profiles/r16_periodic_rows.txt).  Circuit F of tests/rounds_spec.py -- the forward MinRoot round through vdf_cs_repeat --
at t = 2^log2t, advice in device memory.

  (a) the step rate of prove_step_custom under parameters with periodic_rows = 1 against periodic_rows = 0: the same chain proved
      `--runs` times under each, interleaved (A B A B ...) after a warm-up run of each; the proofs are compared byte for byte.
  (b) the kernels alone on a shape made of the circuit's exported triples: k_nifs_cross_periodic plus the OUTSIDE call against the
      single generic vdf_nifs_cross_term call, interleaved, per-launch events summed per call, medians.
  (c) the same rows under vdf_nifs_cross_term_minroot_forward on the built-in forward kind's layout: the distance from the
      hand-written stencil, reported and not bounded.
The run-to-run spread of the GENERIC path against itself (max - min over its runs) is the yardstick: periodic_rows defaults to 1
only if (b) and (a) are faster by more than that."""
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
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_periodic_rows.txt"))
    a = ap.parse_args()
    t = 1 << a.log2t
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "w")

    def out(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    import numpy as np
    import torch
    import vdf_amd
    from rounds_spec import F
    from vdf_amd.minroot import EvalMode, FIELD_FQ, PallasVDF, State
    from vdf_amd.nova import NovaVDFProof, public_params_custom, shape_export_custom, shape_periodic_custom
    out("periodic rows of a custom step circuit (F: the forward MinRoot round through vdf_cs_repeat), t = 2^%d, %d steps; "
        "GPU_MAX_HW_QUEUES = %s" % (a.log2t, a.steps, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    vdf = PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential)
    s = State.from_ints(FIELD_FQ, 123, 0, 0)
    z0, advice = [s.x, s.y, s.i], []
    for _ in range(a.steps):
        s, tr = vdf.eval_with_trace(s, t)
        advice.append(dev(tr))
    # ---- (a) the prover
    circuit = F(t, "repeat")
    pps = {1: public_params_custom(ctx, circuit, periodic_rows=1), 0: public_params_custom(ctx, circuit, periodic_rows=0)}
    rows = pps[1].periodic_rows()
    out("    stencil codes: periodic_rows = 1 -> %d, periodic_rows = 0 -> %d; periodic rows %s of %d constraints" % (
        pps[1].stencil(), pps[0].stencil(), rows, pps[1].sizes()["num_cons"]))

    def run(which):
        proof = None
        ctx.sync()
        t0 = time.perf_counter()
        for adv in advice:
            circuit.advice = adv
            proof = NovaVDFProof.prove_step_custom(pps[which], proof, circuit, z0)
        ctx.sync()
        ms = 1e3 * (time.perf_counter() - t0) / a.steps
        blob = proof.serialize()
        proof.free()
        return ms, blob
    blobs = {w: run(w)[1] for w in (1, 0)}                  # the warm-up
    out("(a) proofs under periodic_rows = 1 and 0 are the same bytes: %s (%d bytes)" % (blobs[1] == blobs[0], len(blobs[1])))
    ms = {1: [], 0: []}
    for _ in range(a.runs):
        for w in (1, 0):
            m, blob = run(w)
            ms[w].append(m)
            assert blob == blobs[w]
    for w in (1, 0):
        out("    periodic_rows = %d: %s ms per step; median %.4f, spread (max - min) %.4f" % (
            w, " ".join("%.4f" % x for x in ms[w]), statistics.median(ms[w]), max(ms[w]) - min(ms[w])))
    gain_a, spread_a = statistics.median(ms[0]) - statistics.median(ms[1]), max(ms[0]) - min(ms[0])
    out("    generic - periodic = %+.4f ms per step; the generic path's own spread is %.4f -> %s" % (
        gain_a, spread_a, "FASTER by more than the spread" if gain_a > spread_a else "no gain beyond the spread"))
    for pp in pps.values():
        pp.free()
    # ---- (b) the kernels alone
    mats = shape_export_custom(circuit)
    pr, info = shape_periodic_custom(circuit)
    nc, ncols = info["num_cons"], info["num_cols"]
    shape = ctx.shape_create(FIELD_FQ, nc, ncols, mats)
    rng = np.random.default_rng(16)

    def rand(n):
        v = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        v[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        return v
    z2 = rand(ncols)
    z2[ncols - 3] = np.frombuffer(State.from_ints(FIELD_FQ, 1, 0, 0).x, dtype="<u8")      # one = 1, as in a fresh instance
    d_in = [dev(z2)] + [dev(rand(nc)) for _ in range(3)]
    u1 = rand(1)
    outs = {k: [torch.zeros((nc, 4), dtype=torch.int64, device="cuda") for _ in range(4)] for k in ("generic", "periodic", "forward")}
    reps = t - pr.lead

    def generic():
        ctx.nifs_cross_term(shape, *d_in, u1, *outs["generic"])

    def periodic():
        ctx.nifs_cross_term_rows(shape, pr.row_begin, pr.row_count, 2, *d_in, u1, *outs["periodic"])
        ctx.nifs_cross_term_periodic(FIELD_FQ, pr, pr.lead, reps, info["seg_begin"], pr.row_begin, ncols, nc, *d_in, u1, *outs["periodic"])

    def forward():       # the hand-written stencil over rows and variables laid out as the built-in kind has them: 3t + 1 rows from the
        #                  repeat's first row, the rounds' variables where the repeat's are (the values are arbitrary: only the time counts)
        ctx.nifs_cross_term_minroot_forward(FIELD_FQ, t, info["seg_begin"], ncols - 3, pr.row_begin - pr.lead * pr.c.n_cons, *d_in, u1,
                                            *outs["forward"])
    variants = {"generic": generic, "periodic": periodic, "forward": forward}
    for f in variants.values():
        f()
    ctx.sync()
    same = all(torch.equal(g, p) for g, p in zip(outs["generic"], outs["periodic"]))
    out("(b) periodic + OUTSIDE writes what the single generic call writes, all %d rows of all four vectors: %s" % (nc, same))
    ctx.set_kernel_timing(True)
    ctx.kernel_events()
    times = {k: [] for k in variants}
    names = {k: set() for k in variants}
    alone = []                                              # k_nifs_cross_periodic without the OUTSIDE call
    for _ in range(a.launches):
        for k, f in variants.items():
            f()
            ctx.sync()
            ev = ctx.kernel_events()
            times[k].append(sum(e[3] - e[2] for e in ev))
            names[k].update(e[0] for e in ev)
            if k == "periodic":
                alone.append(sum(e[3] - e[2] for e in ev if e[0] == "k_nifs_cross_periodic"))
    for k in variants:
        d = times[k][1:]
        out("    %-9s %s: %d calls, kernel time per call median %.4f ms, min %.4f, max %.4f, spread %.4f" % (
            k, "+".join(sorted(names[k])), len(d), statistics.median(d), min(d), max(d), max(d) - min(d)))
    g, p, fw = (statistics.median(times[k][1:]) for k in ("generic", "periodic", "forward"))
    # the spread that counts is the one of medians, not of single launches: the generic path's launches split in two halves
    half = len(times["generic"][1:]) // 2
    g_halves = abs(statistics.median(times["generic"][1:1 + half]) - statistics.median(times["generic"][1 + half:]))
    out("    generic - periodic = %+.4f ms per call (%.2fx); the generic path against itself (medians of its two halves): %.4f -> %s" % (
        g - p, g / p, g_halves, "FASTER by more than the spread" if g - p > g_halves else "no gain beyond the spread"))
    pk = statistics.median(alone[1:])
    out("(c) k_nifs_cross_periodic alone %.4f ms (of the %.4f), the hand-written forward stencil over the same rows %.4f ms: %.2fx" % (
        pk, p, fw, pk / fw))
    shape.free()
    ctx.close()


if __name__ == "__main__":
    main()
