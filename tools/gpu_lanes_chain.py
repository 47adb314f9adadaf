#!/usr/bin/env python3
"""Measurements of the forward step circuit in lanes on one MI355X (output: profiles/r09_lanes.txt by default), profiler off.

  --kernels-only   (a) both lanes kernels at (L, t) = (8, 8192) and (16, 4096) against the single-lane entry points at t = 2^16:
                   the same bytes moved.  Five timed runs each in ONE process (per-launch HIP events of the library), after one
                   warm-up.  Target: the lanes kernel's median does not exceed the single-lane kernel's slowest run.  Beside
                   the L = 1 row through the single-lane entry points, one through the lanes entry points with one lane: in a
                   library that still has single-lane kernels of its own that is what routing one lane through the lanes
                   kernels costs (both medians, and the single-lane runs' own spread); since the single-lane entry points ARE
                   the lanes kernels with one lane, the two rows time the same launch.  Run it
                   under `rocprofv3 --kernel-trace --stats -- python tools/gpu_lanes_chain.py --kernels-only` for the
                   profiler's own figures (a run of its own: output profiles/r09_lanes_kernels.txt).
  (b) step rate:   prove_step/s for L = 4, 8, 16 at L t = 2^16 against VDF_CIRCUIT_MINROOT_FORWARD at t = 2^16, `--steps` steps,
                   `--repeats` alternations in one process after one warm-up alternation; traces resident before the clock
                   starts.  Reported, not gated: every extra lane adds about 1,059 host-synthesised constraints outside the
                   rounds.  Beside it the HBM each parameter set's digit tables took of the budget.
  (c) eight chains of 2^20 rounds end to end, two ways, three interleaved repeats: eight forward proofs at t = 2^16 (16 steps
                   each) with compress_batch and verify_compressed_batch, against ONE lanes proof at (8, 8192) (128 steps) with
                   one compress and one verify.  Wall time of prove + compress + verify, and bytes on the wire.

The chains are made BACKWARDS (vdf_minroot_inverse_eval from an arbitrary end state, three products a round): set-up only.  All
lane counts of (b) read segments of ONE chain of steps x 2^16 rounds with a state kept every 4,096 rounds."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EVERY = 4096


def backward_chain(vdf, State, field, seed, rounds, every=EVERY):
    """states every `every` rounds of a chain of `rounds` rounds, in forward order, made from its END by inverse rounds"""
    s = State.from_ints(field, 0x1234 + seed, 0x77 * seed, rounds + 5 * seed)
    out = [s]
    for _ in range(rounds // every):
        s = vdf.inverse_eval(s, every)
        out.append(s)
    return out[::-1]


def zflat(states):
    return [e for s in states for e in (s.x, s.y, s.i)]


def lanes_circuits(LaneCircuits, t, lane_cps, steps, every=EVERY):
    """a lanes chain of `steps` steps from every lane's checkpoints (lists of State every `every` rounds)"""
    per = t // every
    z0, lc = LaneCircuits.begin(t, [c[0] for c in lane_cps])
    for k in range(steps):
        lc.push_checkpoints(every, [c[k * per:(k + 1) * per + 1] for c in lane_cps])
    return z0, lc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--skip-rate", action="store_true")
    ap.add_argument("--skip-chains", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_lanes.txt"))
    a = ap.parse_args()
    import torch
    import vdf_amd
    from vdf_amd.minroot import EvalMode, FIELD_FQ, PallasVDF, State
    from vdf_amd.nova import (CIRCUIT_MINROOT_FORWARD, LaneCircuits, NovaVDFProof, compress_batch, public_params,
                              public_params_lanes, verify_compressed_batch)
    path = a.out.replace(".txt", "_kernels.txt") if a.kernels_only else a.out
    os.makedirs(os.path.dirname(path), exist_ok=True)
    log = open(path, "w")

    def out(s=""):                                         # every line at once: a run that ends early leaves what it measured
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    ctx = vdf_amd.Context(0)
    vdf = PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential)
    out("forward step circuit in lanes; GPU_MAX_HW_QUEUES = %s" % os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)"))

    if a.kernels_only:
        rng = np.random.default_rng(1)

        def rand(n):
            v = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
            v[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
            return torch.from_numpy(v.view(np.int64)).cuda()
        T = 1 << 16
        u1 = np.ones((1, 4), dtype="<u8")
        runs = {}
        for L, t, single in ((1, T, True), (1, T, False), (8, T // 8, False), (16, T // 16, False)):
            per = 3 * t + 1
            S, nvars = 3 * L + 5, 3 * L + 5 + L * per + 7
            nc, row0 = L * per + 9, 4
            trace = rand(2 * L * (t + 1))
            ends = np.zeros((L, 4), dtype="<u8")
            seg = rand(L * per)
            z2 = rand(nvars + 3)
            abc1 = [rand(nc) for _ in range(3)]
            outs = [rand(nc) for _ in range(4)]
            ctx.set_kernel_timing(True)
            for rep in range(6):
                if single:
                    ctx.minroot_forward_segment(FIELD_FQ, trace, t, ends, seg)
                    ctx.nifs_cross_term_minroot_forward(FIELD_FQ, t, S, nvars, row0, z2, *abc1, u1, *outs)
                else:
                    ctx.minroot_forward_segment_lanes(FIELD_FQ, trace, t + 1, t, L, ends, seg)
                    ctx.nifs_cross_term_minroot_forward_lanes(FIELD_FQ, t, L, S, nvars, row0, z2, *abc1, u1, *outs)
                ctx.sync()
            ev = ctx.kernel_events()
            ctx.set_kernel_timing(False)
            for kind in ("k_forward_segment", "k_nifs_cross_fwd"):
                ms = [e[3] - e[2] for e in ev if e[0].startswith(kind)][1:]          # the first run is the warm-up
                byt = [e[1] for e in ev if e[0].startswith(kind)][0]
                runs[(kind, L, single)] = ms
                out("(a) %-18s %s L = %2d t = %5d  runs (ms) %s  median %.4f  min %.4f  max %.4f  algorithmic bytes %.0f  TB/s at the median %.3f" % (
                    kind, "single-lane entry" if single else "lanes entry      ", L, t, " ".join("%.4f" % x for x in ms), statistics.median(ms), min(ms), max(ms), byt,
                    byt / (statistics.median(ms) * 1e-3) / 1e12))
        for kind in ("k_forward_segment", "k_nifs_cross_fwd"):
            one, slow = runs[(kind, 1, True)], max(runs[(kind, 1, True)])
            out("    %-18s L =  1: median %.4f ms through the single-lane entry (spread of its runs, max - min: %.4f ms), %.4f ms through the lanes entry" % (
                kind, statistics.median(one), slow - min(one), statistics.median(runs[(kind, 1, False)])))
            for L in (8, 16):
                med = statistics.median(runs[(kind, L, False)])
                out("    %-18s L = %2d: median %.4f ms against the single-lane kernel's slowest run %.4f ms: %s" % (
                    kind, L, med, slow, "met" if med <= slow else "NOT met, by %.1f %%" % (100 * (med / slow - 1))))
        ctx.close()
        return

    T = 1 << 16
    # ---- (b) step rate -----------------------------------------------------------------------------------------------
    if not a.skip_rate:
        n = a.steps
        t0 = time.perf_counter()
        chain = backward_chain(vdf, State, FIELD_FQ, 1, n * T)
        out("(b) %d steps; one chain of %d rounds made backwards in %.1f s (set-up), a state every %d rounds" % (n, n * T, time.perf_counter() - t0, EVERY))
        legs = []
        for L in (1, 4, 8, 16):
            t = T // L
            seg = n * t // EVERY                               # checkpoints per lane: lane l is the chain's l-th segment
            cps = [chain[l * seg:(l + 1) * seg + 1] for l in range(L)]
            pp = public_params_lanes(ctx, t, L)
            z0, lc = lanes_circuits(LaneCircuits, t, cps, n)
            lc.materialize(ctx)
            mem = pp.memory()
            out("    L = %2d t = %5d: stencil code %d, primary shape %d x %d, early rows %d; digit tables %s bytes (skipped: %d) of a budget of %d" % (
                L, t, pp.stencil(), pp.sizes(0)["num_cons"], pp.sizes(0)["num_vars"], pp.early_rows()[1], mem["digit_table_bytes"],
                mem["digit_tables_skipped"], pp.tuning()["digit_budget_bytes"]))
            legs.append((L, t, pp, z0, lc, zflat([c[-1] for c in cps])))
        rates = {L: [] for L, *_ in legs}
        for rep in range(a.repeats + 1):                       # one warm-up alternation
            for L, t, pp, z0, lc, zi in legs:
                t0 = time.perf_counter()
                p = NovaVDFProof.prove_recursively(pp, lc, t, z0)
                dt = time.perf_counter() - t0
                if rep == 0:
                    assert p.verify(pp, n, z0, zi), L
                else:
                    rates[L].append(n / dt)
                p.free()
        base = statistics.median(rates[1])
        for L, t, *_ in legs:
            r = rates[L]
            med = statistics.median(r)
            out("    L = %2d t = %5d prove_step/s: %s  median %.1f  min %.1f  max %.1f  (%.4f ms per step; %.3f of the single lane's rate; %.1f chain-steps/s)" % (
                L, t, " ".join("%.1f" % x for x in r), med, min(r), max(r), 1e3 / med, med / base, med * L))
        for L, t, pp, z0, lc, zi in legs:
            lc.free(); pp.free()

    # ---- (c) eight chains of 2^20 rounds, two ways ---------------------------------------------------------------------
    if not a.skip_chains:
        C8, R = 8, 1 << 20
        t0 = time.perf_counter()
        cps = [backward_chain(vdf, State, FIELD_FQ, 10 + c, R) for c in range(C8)]
        out("(c) %d chains of 2^20 rounds made backwards in %.1f s (set-up)" % (C8, time.perf_counter() - t0))
        pp1 = public_params(ctx, T, CIRCUIT_MINROOT_FORWARD)
        pp8 = public_params_lanes(ctx, T // 8, C8)
        singles = []
        for c in range(C8):
            z0, fc = lanes_circuits(LaneCircuits, T, [cps[c]], R // T)
            fc.materialize(ctx)
            singles.append((z0, fc, zflat([cps[c][-1]])))
        z08, l8 = lanes_circuits(LaneCircuits, T // 8, cps, R // (T // 8))
        l8.materialize(ctx)
        zi8 = zflat([c[-1] for c in cps])
        res = {"eight proofs": [], "one lanes proof": []}
        for rep in range(4):                                   # one warm-up alternation
            t0 = time.perf_counter()
            proofs = [NovaVDFProof.prove_recursively(pp1, fc, T, z0) for z0, fc, _ in singles]
            t1 = time.perf_counter()
            snarks = compress_batch(pp1, proofs)
            t2 = time.perf_counter()
            ok = verify_compressed_batch(pp1, [(s, R // T, z0, zi) for s, (z0, _, zi) in zip(snarks, singles)])
            t3 = time.perf_counter()
            assert ok == [True] * C8
            wire = sum(len(s.serialize()) for s in snarks)
            if rep:
                res["eight proofs"].append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, wire))
            for h in snarks + proofs:
                h.free()
            t0 = time.perf_counter()
            p = NovaVDFProof.prove_recursively(pp8, l8, T // 8, z08)
            t1 = time.perf_counter()
            s = p.compress(pp8)
            t2 = time.perf_counter()
            ok = s.verify(pp8, R // (T // 8), z08, zi8)
            t3 = time.perf_counter()
            assert ok
            wire = len(s.serialize())
            if rep:
                res["one lanes proof"].append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, wire))
            s.free(); p.free()
        tot, wires = {}, {name: rows[0][3] for name, rows in res.items()}
        for name, rows in res.items():
            for r in rows:
                out("    %-16s prove %.1f ms  compress %.1f ms  verify %.1f ms  total %.1f ms  wire %d bytes" % (name, r[0], r[1], r[2], sum(r[:3]), r[3]))
            tot[name] = statistics.median(sum(r[:3]) for r in rows)
            part = [statistics.median(r[k] for r in rows) for k in range(3)]
            out("    %-16s medians: prove %.1f  compress %.1f  verify %.1f  total %.1f ms" % (name, part[0], part[1], part[2], tot[name]))
            res[name] = part
        out("    one lanes proof / eight proofs: %.3f of the wall time, %.3f of the bytes" % (
            tot["one lanes proof"] / tot["eight proofs"], wires["one lanes proof"] / wires["eight proofs"]))
        # the chain length at which both ways cost the same: prove scales with the rounds, compress + verify do not
        e, l = res["eight proofs"], res["one lanes proof"]
        per_round_gap = (l[0] - e[0]) / R                      # what the lanes way pays more per round of every chain
        fixed_gain = (e[1] + e[2]) - (l[1] + l[2])             # what it saves whatever the length
        if per_round_gap > 0 and fixed_gain > 0:
            out("    break-even: the lanes way pays %.3f us more per round and saves %.1f ms per batch of eight: equal cost at %.0f rounds per chain (2^%.1f)" % (
                per_round_gap * 1e3, fixed_gain, fixed_gain / per_round_gap, np.log2(fixed_gain / per_round_gap)))
        else:
            out("    break-even: none in this run (per-round gap %.3f us, fixed gain %.1f ms)" % (per_round_gap * 1e3, fixed_gain))
        for z0, fc, _ in singles:
            fc.free()
        l8.free(); pp1.free(); pp8.free()
    ctx.close()


if __name__ == "__main__":
    main()
