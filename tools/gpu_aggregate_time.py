"""Aggregating K running proofs into one compressed proof against compressing and verifying them as a batch, at t = 2^16 on the
reference's circuit: K in {1, 2, 4, 8, 16} proofs of 4 steps each, distinct chains, in one process.  Per K and quantity the median,
minimum and maximum over the repeats, the two ways taking turns repeat by repeat:
  batch      make   = vdf_nova_compress_batch + vdf_nova_snark_serialize of every proof
             verify = vdf_nova_verify_wire_batch over the same bytes
  aggregate  make   = vdf_nova_compress_aggregate + vdf_nova_aggregate_serialize
             verify = vdf_nova_aggregate_deserialize + vdf_nova_verify_aggregate
  bytes of both ways, and the kernel events (KTimer) of k_cross_term_relaxed and k_fold_relaxed of one aggregation, beside
  k_cross_term over the same rows (vdf_cross_term on the accumulator's vectors would read 7 of the same 32-byte streams).
No threshold: the figures are the result.  The claim of aggregation is bytes and verifier time per proof for K > 1.
usage: python tools/gpu_aggregate_time.py [--lg 16] [--ks 1,2,4,8,16] [--steps 4] [--repeats 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
from gpu_verify_multi_time import kernel_figures  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=16)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import vdf_amd
    from oracle import pasta as o
    from vdf_amd import _lib
    from vdf_amd.minroot import EvalMode, PallasVDF, State, FIELD_FQ
    from vdf_amd.nova import (InverseMinRootCircuit, NovaVDFProof, compress_aggregate, compress_batch, deserialize_aggregate, public_params,
                              verify_wire_batch)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t, n = 1 << a.lg, a.steps
    ks = [int(x) for x in a.ks.split(",") if x]
    ctx = vdf_amd.Context(0)
    pp = public_params(ctx, t)
    items = []
    for q in range(max(ks)):
        init = State.from_ints(FIELD_FQ, o.rand_fe(9000 + q, 0, o.Q), 0, 1)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential), t, n, init)
        items.append((NovaVDFProof.prove_recursively(pp, circuits, t, z0), n, z0, [init.x, init.y, init.i]))
    say(f"t = 2^{a.lg}, {n} steps per proof, {a.repeats} alternating repeats in one process; ms as median [min .. max]")
    fmt = lambda v: "%8.2f [%8.2f .. %8.2f]" % (statistics.median(v), min(v), max(v))
    for K in ks:
        its = items[:K]
        proofs = [it[0] for it in its]
        stmt = ([it[1] for it in its], [it[2] for it in its], [it[3] for it in its])
        blobs = [s.serialize() for s in compress_batch(pp, proofs)]                  # warm both ways
        agg_bytes = compress_aggregate(pp, proofs).serialize()
        tm = {k: [] for k in ("batch make", "batch verify", "aggregate make", "aggregate verify")}
        for _ in range(a.repeats):
            ctx.sync(); t0 = time.perf_counter()
            snarks = compress_batch(pp, proofs); blobs = [s.serialize() for s in snarks]; ctx.sync()
            tm["batch make"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            agg = compress_aggregate(pp, proofs); agg_bytes = agg.serialize(); ctx.sync()
            tm["aggregate make"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            res = verify_wire_batch(pp, [(b,) + it[1:] for b, it in zip(blobs, its)]); ctx.sync()
            tm["batch verify"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            verdict = deserialize_aggregate(pp, agg_bytes).verify(pp, *stmt); ctx.sync()
            tm["aggregate verify"].append(1e3 * (time.perf_counter() - t0))
            if not all(ok for ok, _ in res) or verdict != (True, -1):
                sys.exit(f"K = {K}: a proof does not verify")
            for s in snarks:
                s.free()
            agg.free()
        say(f"K = {K:2d}   bytes: batch {sum(len(b) for b in blobs)}  aggregate {len(agg_bytes)}")
        for k, v in tm.items():
            say(f"   {k:17s} ms {fmt(v)}   per proof {statistics.median(v) / K:8.2f}")
        # the two kernels of one aggregation of these K proofs, from the library's events
        ctx.set_kernel_timing(True)
        ctx.kernel_events()
        compress_aggregate(pp, proofs).free()
        ctx.sync()
        ev = ctx.kernel_events()
        ctx.set_kernel_timing(False)
        for name in ("k_cross_term_relaxed", "k_fold_relaxed"):
            for rows in sorted({int(b / (224 if name == "k_cross_term_relaxed" else 416)) for kn, b, _, _ in ev if kn == name}):
                us = [1e3 * (e1 - e0) for kn, b, e0, e1 in ev if kn == name and int(b / (224 if name == "k_cross_term_relaxed" else 416)) == rows]
                say(f"   {name:21s} {rows:8d} rows: {len(us):3d} launches, us {statistics.median(us):7.1f} [{min(us):7.1f} .. {max(us):7.1f}]")
    # k_cross_term beside them, on the rows of the primary side's accumulator
    rows = pp.sizes(0)["num_cons"]
    if rows:
        rng = np.random.default_rng(1)
        mk = lambda: torch.from_numpy((rng.integers(0, 2**62, size=(rows, 4), dtype=np.uint64)).view(np.int64)).cuda()
        v = [mk() for _ in range(7)]
        u = np.zeros((1, 4), dtype="<u8"); u[0, 0] = 1
        ctx.set_kernel_timing(True)
        ctx.kernel_events()
        for _ in range(9):
            ctx.cross_term(FIELD_FQ, v[0], v[1], v[2], v[3], v[4], v[5], u, rows, v[6])
            ctx.cross_term_relaxed(FIELD_FQ, v[0], v[1], v[2], u, v[3], v[4], v[5], u, rows, v[6])
        ctx.sync()
        ev = ctx.kernel_events()
        ctx.set_kernel_timing(False)
        for name in ("k_cross_term", "k_cross_term_relaxed"):
            us = [1e3 * (e1 - e0) for kn, _, e0, e1 in ev if kn == name][1:]
            say(f"side by side on {rows} rows: {name:21s} us {statistics.median(us):7.1f} [{min(us):7.1f} .. {max(us):7.1f}]")
    for name in ("k_cross_term_relaxed", "k_fold_relaxed"):
        for sym, vgpr, agpr, lds, scratch in kernel_figures(_lib.lib._name, name):
            say(f"{sym}: {vgpr} VGPRs, {agpr} AGPRs, {lds} B LDS, {scratch} B scratch")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
