#!/usr/bin/env python3
"""Measurements of custom chains in lanes (vdf_round_tape_walk_lanes, vdf_cs_repeat_lanes, vdf_nova_custom_chain_lanes_from_checkpoints)
on one MI355X, profiler off (output: profiles/r18_custom_lanes.txt).  ONE process; every comparison is made in alternating
repeats over the same buffers.  Every figure is reported, none is gated.

  (a) one walks launch against L launches.  t = 2^16, checkpoints every 4,096 rounds, W = 16 steps, L = 8 and 16 lanes: one
      vdf_round_tape_walk_lanes slice of 1,024 rounds over all W * L * 16 walks, against L launches of vdf_round_tape_walk over the
      same walks and the same trace (the arrangement the single call allows), and one of those L launches alone.  Wall time from
      the first enqueue to the end of the queue.
  (b) steps per second of prove_recursively_custom for L = 1, 4, 8, 16 lanes at L * t = 2^16 (the same rounds per step).
  (c) eight chains of 2^20 rounds end to end: eight custom proofs (t = 8,192, 128 steps each) with compress_batch and
      verify_compressed_batch, against ONE lanes proof at (8, 8,192).  Wall time of proving, compressing and verifying, and the
      bytes on the wire."""
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
    ap.add_argument("--steps", type=int, default=32, help="steps of (b)")
    ap.add_argument("--log2rounds", type=int, default=20, help="rounds per chain of (c)")
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_custom_lanes.txt"))
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
    from vdf_amd.minroot import FIELD_FQ, PallasVDF, State
    from vdf_amd.nova import (CustomChain, NovaVDFProof, compress_batch, public_params_custom, record_walk_body, verify_compressed_batch)
    from custom_chain_spec import FC
    from custom_lanes_spec import FL
    from walks_spec import minroot_body
    from util import dev, states_array
    out("custom chains in lanes, %d alternating repeats; GPU_MAX_HW_QUEUES = %s" % (a.runs, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    walk_tape = record_walk_body(minroot_body(FIELD_FQ))
    med = statistics.median

    def backwards(seed, intervals, every, i_last):
        """a chain's checkpoints from an arbitrary last state (the inverse round is cheap): [State] of intervals + 1, forward order"""
        cps = [State.from_ints(FIELD_FQ, 0x123456789ABCDEF + seed, 0xFEDCBA987654321 + 3 * seed, i_last)]
        for _ in range(intervals):
            cps.insert(0, PallasVDF.inverse_eval(cps[0], every))
        return cps

    # ---- (a) ------------------------------------------------------------------------------------------------------------------
    if "a" in a.parts:
        t, every, W, rounds = 1 << 16, 4096, 16, 1024
        per = t // every
        for L in (8, 16):
            n = W * L * per
            rng = np.random.default_rng(L)
            starts = rng.integers(0, 2**62, size=(n * 2, 4)).astype("<u8")
            starts[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
            d_start = dev(starts)
            d_trace = torch.zeros((W * L * (t + 1) * 2, 4), dtype=torch.int64, device="cuda")
            inv = starts[:L].copy()
            j_base = [1000 * l for l in range(L)]
            lane_of = (np.arange(n) // per) % L
            d_lane = [dev(starts.reshape(n, 8)[lane_of == l].reshape(-1, 4)) for l in range(L)]

            def one():
                e = d_start.clone()
                torch.cuda.synchronize()                        # (the copy runs on torch's stream, the walks on the context's)
                ctx.sync()
                t0 = time.perf_counter()
                ctx.round_tape_walk_lanes(FIELD_FQ, walk_tape, L, inv, e, n, rounds, d_trace, walk_stride=every, top=every, group=per,
                                          group_stride=t + 1, j_base=j_base, j_group_step=t)
                ctx.sync()
                return 1e3 * (time.perf_counter() - t0), e

            def many(lanes):
                es = [d_lane[l].clone() for l in lanes]
                torch.cuda.synchronize()
                ctx.sync()
                t0 = time.perf_counter()
                for e, l in zip(es, lanes):
                    ctx.round_tape_walk(FIELD_FQ, walk_tape, inv[l:l + 1], e, W * per, rounds, d_trace[2 * l * (t + 1):], walk_stride=every, top=every,
                                        group=per, group_stride=L * (t + 1), j_base=j_base[l], j_group_step=t)
                ctx.sync()
                return 1e3 * (time.perf_counter() - t0), es
            ms1, e1 = one()
            tr1 = d_trace.clone()
            d_trace.zero_()
            torch.cuda.synchronize()
            _, es = many(range(L))
            got = torch.empty_like(e1).view(n, 8)
            for l in range(L):
                got[torch.from_numpy(lane_of == l).cuda()] = es[l].view(-1, 8)
            assert torch.equal(got.view(-1, 4), e1) and torch.equal(tr1, d_trace), "the two arrangements differ"
            del tr1, got
            r = {"one": [], "many": [], "single": []}
            for _ in range(a.runs):
                r["one"].append(one()[0])
                r["many"].append(many(range(L))[0])
                r["single"].append(many([0])[0])
            out("(a) L = %-2d W = %d, %d walks, a slice of %d rounds: ONE vdf_round_tape_walk_lanes  %s ms  median %.3f | %d launches of "
                "vdf_round_tape_walk  %s ms  median %.3f | one of them alone (%d walks)  %s ms  median %.3f | one launch / L launches = %.3f, "
                "one launch / a single lane's = %.3f" % (
                    L, W, n, rounds, " ".join("%.3f" % x for x in r["one"]), med(r["one"]), L, " ".join("%.3f" % x for x in r["many"]), med(r["many"]),
                    W * per, " ".join("%.3f" % x for x in r["single"]), med(r["single"]), med(r["one"]) / med(r["many"]), med(r["one"]) / med(r["single"])))
            del d_trace, d_start, d_lane
            torch.cuda.empty_cache()

    def lanes_setup(L, t, every, steps):
        """(chain, z0, zi, circuit, parameters) of L lanes of `steps` steps"""
        per = t // every
        lanes_cps = [backwards(l, steps * per, every, 7 + 1000 * l + steps * t) for l in range(L)]
        arr = np.concatenate([np.ascontiguousarray(states_array(c)[:, :8]).reshape(-1, 4) for c in lanes_cps])
        inv = np.concatenate([np.ascontiguousarray(states_array(c)[0, 8:12]).reshape(1, 4) for c in lanes_cps])
        z0 = [v for c in lanes_cps for v in (c[0].x, c[0].y, c[0].i)]
        zi = [v for c in lanes_cps for v in (c[-1].x, c[-1].y, c[-1].i)]
        chain = CustomChain.lanes_from_checkpoints(FIELD_FQ, walk_tape, inv, t, every, steps, L, arr)
        c = FL(t, L)
        return chain, z0, zi, c, public_params_custom(ctx, c)

    # ---- (b) ------------------------------------------------------------------------------------------------------------------
    if "b" in a.parts:
        sets = {}
        for L in (1, 4, 8, 16):
            t = (1 << 16) // L
            sets[L] = lanes_setup(L, t, min(4096, t), a.steps)
        rates = {L: [] for L in sets}

        def prove(L):
            chain, z0, zi, c, pp = sets[L]
            ctx.sync()
            t0 = time.perf_counter()
            proof = NovaVDFProof.prove_recursively_custom(pp, c, chain, z0, window_steps=16)
            ctx.sync()
            dt = time.perf_counter() - t0
            assert proof.verify(pp, a.steps, z0, zi) is True
            proof.free()
            return a.steps / dt
        for L in sets:
            prove(L)                                            # once untimed: allocations, tables, the side queue
        for _ in range(a.runs):
            for L in sets:
                rates[L].append(prove(L))
        for L in sets:
            r = rates[L]
            out("(b) L = %-2d t = %-5d (L * t = 2^16), %d steps, W = 16: steps/s  %s  median %.1f, min %.1f, max %.1f; chains x rounds per second %.0f" % (
                L, (1 << 16) // L, a.steps, " ".join("%.1f" % x for x in r), med(r), min(r), max(r), med(r) * (1 << 16)))
        for chain, _, _, _, pp in sets.values():
            chain.free(); pp.free()

    # ---- (c) ------------------------------------------------------------------------------------------------------------------
    if "c" in a.parts:
        L, t, every = 8, 8192, 4096
        steps = (1 << a.log2rounds) // t
        chain, z0, zi, c, pp = lanes_setup(L, t, every, steps)
        c1 = FC(t)
        pp1 = public_params_custom(ctx, c1)
        per = t // every
        singles = []
        for l in range(L):
            cps = backwards(l, steps * per, every, 7 + 1000 * l + steps * t)
            arr = states_array(cps)
            singles.append((CustomChain.from_checkpoints(FIELD_FQ, walk_tape, np.ascontiguousarray(arr[0, 8:12]).reshape(1, 4), t, every, steps,
                                                         np.ascontiguousarray(arr[:, :8]).reshape(-1, 4)),
                            [cps[0].x, cps[0].y, cps[0].i], [cps[-1].x, cps[-1].y, cps[-1].i]))

        def eight():
            ctx.sync()
            t0 = time.perf_counter()
            proofs = [NovaVDFProof.prove_recursively_custom(pp1, c1, ch, z, window_steps=16) for ch, z, _ in singles]
            t1 = time.perf_counter()
            snarks = compress_batch(pp1, proofs)
            t2 = time.perf_counter()
            wire = [s.serialize() for s in snarks]
            ok = verify_compressed_batch(pp1, [(s, steps, z, zz) for s, (_, z, zz) in zip(snarks, singles)])
            t3 = time.perf_counter()
            assert all(ok)
            for x in snarks + proofs:
                x.free()
            return 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), sum(len(w) for w in wire)

        def one():
            ctx.sync()
            t0 = time.perf_counter()
            proof = NovaVDFProof.prove_recursively_custom(pp, c, chain, z0, window_steps=16)
            t1 = time.perf_counter()
            snark = proof.compress(pp)
            t2 = time.perf_counter()
            wire = snark.serialize()
            ok = snark.verify(pp, steps, z0, zi)
            t3 = time.perf_counter()
            assert ok is True
            snark.free(); proof.free()
            return 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), len(wire)
        eight(); one()                                          # once untimed
        r8, r1 = [], []
        for _ in range(a.runs):
            r8.append(eight())
            r1.append(one())
        for name, r in (("eight proofs (t = %d, %d steps each), compress_batch, verify_compressed_batch" % (t, steps), r8),
                        ("ONE lanes proof (8 lanes, t = %d, %d steps), compress, verify_compressed" % (t, steps), r1)):
            tot = [x[0] + x[1] + x[2] for x in r]
            out("(c) %-84s prove %.1f ms, compress %.1f ms, verify %.1f ms (medians); end to end %s ms  median %.1f; %d bytes on the wire" % (
                name, med(x[0] for x in r), med(x[1] for x in r), med(x[2] for x in r), " ".join("%.1f" % x for x in tot), med(tot), r[0][3]))
        for ch, _, _ in singles:
            ch.free()
        chain.free(); pp.free(); pp1.free()
    ctx.close()


if __name__ == "__main__":
    main()
