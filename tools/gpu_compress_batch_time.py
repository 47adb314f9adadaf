"""compress_batch against single compress calls at t = 2^k (default 16), reference circuit: for K in {1, 2, 4, 8} proofs of
two steps each, warm, the batch and K single calls interleaved in one process (best of --reps), every output compared
byte for byte.  Prints per-proof milliseconds of both.  --trace-k K: after the table, one more batch of K proofs
(for a rocprofv3 --kernel-trace --stats run around it)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vdf_amd
from vdf_amd.minroot import PallasVDF, State, FIELD_FQ, EvalMode
from vdf_amd.nova import InverseMinRootCircuit, NovaVDFProof, compress_batch, public_params, verify_compressed_batch

ap = argparse.ArgumentParser()
ap.add_argument("--lg", type=int, default=16)
ap.add_argument("--ks", default="1,2,4,8")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--trace-k", type=int, default=0)
a = ap.parse_args()
t, n = 1 << a.lg, 2
ks = [int(x) for x in a.ks.split(",") if x]
ctx = vdf_amd.Context(0)
pp = public_params(ctx, t)
items = []
for q in range(max(ks + [a.trace_k])):
    initial = State.from_ints(FIELD_FQ, 4242 + q, 0, 0)
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential), t, n, initial)
    items.append((NovaVDFProof.prove_recursively(pp, circuits, t, z0), n, z0, [initial.x, initial.y, initial.i]))
proofs = [it[0] for it in items]
print(f"t = 2^{a.lg}, {n} steps per proof, best of {a.reps} (per-proof ms)")
print("%3s %10s %10s %8s" % ("K", "batch", "single", "speedup"))
for k in ks:
    ps = proofs[:k]
    compress_batch(pp, ps)                                             # warm: the groups' queues and scratch
    for p in ps:
        p.compress(pp).free()
    best_b = best_s = float("inf")
    for _ in range(a.reps):
        t0 = time.perf_counter(); got = compress_batch(pp, ps); ctx.sync(); tb = time.perf_counter() - t0
        t0 = time.perf_counter(); one = [p.compress(pp) for p in ps]; ctx.sync(); ts = time.perf_counter() - t0
        best_b, best_s = min(best_b, tb), min(best_s, ts)
        for g, s in zip(got, one):
            if g.serialize() != s.serialize():
                sys.exit(f"K = {k}: batch output differs from single compress")
    ok = verify_compressed_batch(pp, [(g,) + it[1:] for g, it in zip(got, items)])
    if not all(ok):
        sys.exit(f"K = {k}: a batch output does not verify")
    print("%3d %10.2f %10.2f %7.2fx" % (k, 1e3 * best_b / k, 1e3 * best_s / k, best_s / best_b), flush=True)
if a.trace_k:
    ctx.sync()
    t0 = time.perf_counter(); compress_batch(pp, proofs[:a.trace_k]); ctx.sync()
    print(f"traced batch of {a.trace_k}: {1e3 * (time.perf_counter() - t0):.1f} ms")
