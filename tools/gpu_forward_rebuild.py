#!/usr/bin/env python3
"""Measurements of traces rebuilt by forward tapes (vdf_round_tape_rebuild_lanes, the ascending vdf_custom_chain) on one MI355X,
profiler off (output: profiles/r24_forward_rebuild.txt).  ONE process; every comparison is made in alternating repeats.  Every
figure is reported, none is gated.

  (a) the kernel.  k_tape_rebuild_lanes against vdf_round_tape_forward_walk with `trace` on (k_tape_forward_walk_chain): the same
      tape (the MinRoot forward round with the library's addition chain), the same 2^16 walks, 64 rounds, the same trace layout.
      Wall time from the enqueue to the end of the queue; the two traces are compared byte for byte.  The interpreter is shared and
      only the indexing differs: the ratio is expected near 1.0, and whatever it is is printed.
  (b) the prover.  prove_recursively_custom at t = 2^16, 64 steps, W = 32, checkpoints every 64, 256 and 4,096 rounds: an ASCENDING
      chain (the forward tape) against a DESCENDING chain of the same function (its walk tape: five products a round) in the same
      run, and against the vdf_nova_prove_step_custom loop over a ready host trace uploaded per step.  MinRoot has a cheap inverse:
      the comparison says what a round WITHOUT one pays for checkpoints in the place of traces."""
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--log2t", type=int, default=16)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--every", default="64,256,4096")
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_forward_rebuild.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "w")

    def out(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    import numpy as np
    import torch
    import vdf_amd
    from vdf_amd.minroot import FIELD_FQ, PallasVDF, State, pow_chain
    from vdf_amd.nova import CustomChain, NovaVDFProof, WalkBody, public_params_custom, record_forward_body, record_walk_body
    from custom_chain_spec import FC
    from walks_spec import minroot_body
    from util import dev, dev_read, states_array
    out("traces rebuilt by forward tapes, %d alternating repeats; GPU_MAX_HW_QUEUES = %s" % (a.runs, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    chain5 = pow_chain(FIELD_FQ)
    # x' = (x + y)^(1/5) by the library's chain, y' = x + i0 + j: the round walks_spec.minroot_body inverts
    fwd = record_forward_body(WalkBody(1, 2, lambda cs, j, inv, cur: [cs.pow_chain(cs.add(cur[0], cur[1]), chain5), cs.add(cur[0], cs.add(inv[0], j))]), FIELD_FQ)
    walk = record_walk_body(minroot_body(FIELD_FQ), FIELD_FQ)
    med = statistics.median

    # ---- (a) ------------------------------------------------------------------------------------------------------------------
    if "a" in a.parts:
        n, rounds = 1 << 16, 64
        rng = np.random.default_rng(1)
        starts = rng.integers(0, 2**62, size=(n * 2, 4)).astype("<u8")
        starts[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
        inv = starts[:1].copy()
        d_start = dev(starts)
        tr = [torch.zeros((n * (rounds + 1) * 2, 4), dtype=torch.int64, device="cuda") for _ in range(2)]

        def rebuild():
            e = d_start.clone()
            torch.cuda.synchronize()
            ctx.sync()
            t0 = time.perf_counter()
            ctx.round_tape_rebuild_lanes(FIELD_FQ, fwd, 1, inv, e, n, rounds, trace=tr[0], walk_stride=rounds + 1, base=0, group=0, j_base=[0], j_group_step=0)
            ctx.sync()
            return 1e3 * (time.perf_counter() - t0), e

        def forward():
            e = d_start.clone()
            torch.cuda.synchronize()
            ctx.sync()
            t0 = time.perf_counter()
            ctx.round_tape_forward_walk(FIELD_FQ, fwd, inv, e, n, rounds, trace=tr[1], walk_stride=rounds + 1, base=0, j_base=0, j_walk_step=rounds + 1)
            ctx.sync()
            return 1e3 * (time.perf_counter() - t0), e
        (_, e0), (_, e1) = rebuild(), forward()
        assert torch.equal(e0, e1) and torch.equal(tr[0], tr[1]), "the two kernels differ"
        r = {"rebuild": [], "forward": []}
        for _ in range(a.runs):
            r["rebuild"].append(rebuild()[0])
            r["forward"].append(forward()[0])
        out("(a) %d walks x %d rounds, trace on: k_tape_rebuild_lanes  %s ms  median %.3f (%.1f us per round and lane) | k_tape_forward_walk_chain  "
            "%s ms  median %.3f (%.1f us) | rebuild / forward = %.4f; entries and traces byte for byte equal" % (
                n, rounds, " ".join("%.3f" % x for x in r["rebuild"]), med(r["rebuild"]), 1e3 * med(r["rebuild"]) / rounds,
                " ".join("%.3f" % x for x in r["forward"]), med(r["forward"]), 1e3 * med(r["forward"]) / rounds, med(r["rebuild"]) / med(r["forward"])))
        del tr, d_start
        torch.cuda.empty_cache()

    # ---- (b) ------------------------------------------------------------------------------------------------------------------
    if "b" in a.parts:
        t, steps, W = 1 << a.log2t, a.steps, a.window
        everys = sorted(int(v) for v in a.every.split(","))
        fine = everys[0]
        # the chain's checkpoints every `fine` rounds, built downwards from an arbitrary last state (the inverse round is cheap)
        i_first = 7
        cps = [State.from_ints(FIELD_FQ, 0x123456789ABCDEF, 0xFEDCBA987654321, i_first + steps * t)]
        for _ in range(steps * t // fine):
            cps.append(PallasVDF.inverse_eval(cps[-1], fine))
        cps.reverse()
        arr = states_array(cps)
        xy = np.ascontiguousarray(arr[:, :8]).reshape(-1, 2, 4)
        inv = np.ascontiguousarray(arr[0, 8:12]).reshape(1, 4)
        z0, zi = [cps[0].x, cps[0].y, cps[0].i], [cps[-1].x, cps[-1].y, cps[-1].i]
        c = FC(t)
        pp = public_params_custom(ctx, c)

        def chain_of(every, forward):
            sub = np.ascontiguousarray(xy[::every // fine]).reshape(-1, 4)
            return CustomChain.from_checkpoints(FIELD_FQ, fwd if forward else walk, inv, t, every, steps, sub, forward=forward)
        # the ready host traces: every step's, by the descending chain once (untimed)
        ch = chain_of(everys[-1], False)
        traces = []
        for g in range(steps):
            ch.materialize(ctx, g, 1)
            traces.append(dev_read(ctx, ch.advice(g), (t + 1) * 64).reshape(-1, 4))
            ch.release(g, 1)
        ch.free()

        def recursively(chain):
            ctx.sync()
            t0 = time.perf_counter()
            proof = NovaVDFProof.prove_recursively_custom(pp, c, chain, z0, window_steps=W)
            ctx.sync()
            dt = time.perf_counter() - t0
            return proof, dt

        def by_steps():
            ctx.sync()
            t0 = time.perf_counter()
            proof = None
            for g in range(steps):
                c.advice = traces[g]
                proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
            ctx.sync()
            dt = time.perf_counter() - t0
            c.advice = None
            return proof, dt
        proof, _ = by_steps()                                   # once untimed; and the bytes every arrangement must give
        assert proof.verify(pp, steps, z0, zi) is True
        want = proof.serialize()
        proof.free()
        for every in everys:
            up, down = chain_of(every, True), chain_of(every, False)
            for chain in (up, down):                            # once untimed: the side queue, the buffers
                proof, _ = recursively(chain)
                assert proof.serialize() == want, "the proof differs"
                proof.free()
            r = {"up": [], "down": [], "host": []}
            for _ in range(a.runs):
                for key, run in (("up", lambda: recursively(up)), ("down", lambda: recursively(down)), ("host", by_steps)):
                    proof, dt = run()
                    proof.free()
                    r[key].append(1e3 * dt / steps)
            out("(b) t = 2^%d, %d steps, W = %d, every = %-5d (at most %d rounds per launch): ms per step  ASCENDING  %s  median %.3f | DESCENDING  %s  "
                "median %.3f | host trace per step  %s  median %.3f | ascending / descending = %.2f, ascending / host trace = %.2f; checkpoints "
                "held %.1f KiB, one window of traces %.1f MiB" % (
                    a.log2t, steps, W, every, up.launch_rounds(0), " ".join("%.3f" % x for x in r["up"]), med(r["up"]),
                    " ".join("%.3f" % x for x in r["down"]), med(r["down"]), " ".join("%.3f" % x for x in r["host"]), med(r["host"]),
                    med(r["up"]) / med(r["down"]), med(r["up"]) / med(r["host"]), (steps * t // every + 1) * 64 / 1024.0, W * (t + 1) * 64 / 2.0**20))
            up.free(); down.free()
        pp.free()
    ctx.close()


if __name__ == "__main__":
    main()
