"""Verifying compressed proofs from their wire bytes, at t = 2^16: 16 proofs of distinct chains, serialised once, in one
process; batches of K = 1, 2, 4, 8, 16; per K and quantity the minimum, median and maximum ms per proof over the repeats, the
quantities taking turns repeat by repeat:
  (a) a loop of vdf_nova_snark_deserialize calls (every point decoded on the host)
  (b) vdf_nova_snark_deserialize_batch (every point decoded on the device, one launch per curve)
  (c) the loop of (a), then vdf_nova_verify_compressed_batch over the handles
  (d) vdf_nova_verify_wire_batch
  (e) k_points_decompress alone, from the HIP events the library puts around its launches (KTimer), one batch of each K
  (f) the number of points a proof carries
and the new kernels' registers, LDS and scratch from the library's code object.

The baseline is never the code under test: run the same file on a built checkout of the parent commit with --root (it has
neither batch call, and its host root recomputes 5^T on every call: it gives (a) and (c) as that commit has them), in the same
session, and keep the records side by side:
  python tools/gpu_wire_batch_time.py --root /path/to/parent/checkout --out parent.txt
  python tools/gpu_wire_batch_time.py --out this.txt
A build whose decoder runs the generators' data-dependent root instead of the fixed-trip one (make ab
AB_FLAGS=-DVDF_POINTS_SQRT_VARTIME) is timed with VDF_HIP_LIB set to it; --kernel-only then skips (a)-(d).
usage: python tools/gpu_wire_batch_time.py [--lg 16] [--proofs 16] [--repeats 5] [--root DIR] [--kernel-only] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from gpu_verify_multi_time import kernel_figures  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import vdf_amd
    from oracle import pasta as o
    from vdf_amd import _lib, nova
    from vdf_amd.minroot import PallasVDF, State, FIELD_FQ
    from vdf_amd.nova import CompressedNovaVDFProof, InverseMinRootCircuit, NovaVDFProof, public_params, verify_compressed_batch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t, P = 1 << a.lg, a.proofs
    ctx = vdf_amd.Context(0)
    pp = public_params(ctx, t)
    has_batch = hasattr(nova, "verify_wire_batch")
    items, t0 = [], time.perf_counter()
    for q in range(P):
        x = o.rand_fe(8000 + q, 0, o.Q)
        init = State.from_ints(FIELD_FQ, x, 0, 1)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, a.steps, init)
        snark = NovaVDFProof.prove_recursively(pp, circuits, t, z0).compress(pp)
        items.append((snark.serialize(), a.steps, z0, [init.x, init.y, init.i]))
        flat = len(snark.to_bytes())
        snark.free()
    wire = len(items[0][0])
    header = 48 + 5 * 32 * 2 + 3 * 32 + 32 + 128
    points = 6 + (flat - (wire - header)) // 32          # five instance commitments and T2; an argument's point is 64 bytes flat, 32 on the wire
    here = os.path.abspath(a.root) == HERE
    say(f"library {os.path.relpath(_lib.LIB_PATH, os.path.abspath(a.root))} of {'this checkout' if here else 'the checkout given with --root'}"
        + ("" if has_batch else " (no batch calls: the baseline)"))
    say(f"t = 2^{a.lg}: {P} compressed proofs of distinct chains ({a.steps} steps each) made and serialised in {time.perf_counter() - t0:.1f} s; "
        f"{wire} bytes and (f) {points} points per proof; {a.repeats} repeats per figure, the quantities taking turns; ms per proof")

    def loop(batch):
        return [(CompressedNovaVDFProof.deserialize(pp, blob), n, z0, zi) for blob, n, z0, zi in batch]

    def free(handles):
        for h in handles:
            h[0].free()

    def qa(batch):
        free(loop(batch))

    def qb(batch):
        got = nova.deserialize_compressed_batch(pp, [it[0] for it in batch])
        assert all(status == 0 for _, status in got)
        free(got)

    def qc(batch):
        hs = loop(batch)
        assert verify_compressed_batch(pp, hs) == [True] * len(batch)
        free(hs)

    def qd(batch):
        assert nova.verify_wire_batch(pp, batch) == [(True, 0)] * len(batch)

    names = {"a": "(a) deserialize, a loop", "b": "(b) deserialize_batch", "c": "(c) loop + verify_compressed_batch", "d": "(d) verify_wire_batch"}
    run = {"a": qa, "c": qc}
    if has_batch:
        run.update({"b": qb, "d": qd})
    order = [k for k in "abcd" if k in run]
    res = {}
    if not a.kernel_only:
        for k in order:                                  # warm-up of every shape and allocation the timed window uses
            run[k](items)
        say("  %-4s %-38s %9s %9s %9s" % ("K", "quantity", "min", "median", "max"))
        for b in (1, 2, 4, 8, 16):
            if b > P:
                break
            reps = {k: [] for k in order}
            for _ in range(a.repeats):
                for k in order:
                    ctx.sync()
                    t0 = time.perf_counter()
                    run[k](items[:b])
                    reps[k].append((time.perf_counter() - t0) * 1e3 / b)
            for k in order:
                res[b, k] = (min(reps[k]), statistics.median(reps[k]), max(reps[k]))
                say("  %-4d %-38s %9.3f %9.3f %9.3f" % ((b, names[k]) + res[b, k]))

    if has_batch:
        say()
        say("(e) k_points_decompress by events, both curves' launches of one vdf_nova_snark_deserialize_batch; ms per batch, and per point in us")
        qb(items)
        for b in (1, 2, 4, 8, 16):
            if b > P:
                break
            ms = []
            for _ in range(a.repeats):
                ctx.sync()
                ctx.set_kernel_timing(True)
                ctx.kernel_events()
                qb(items[:b])
                ctx.sync()
                ev = ctx.kernel_events()
                ctx.set_kernel_timing(False)
                mine = [(s1 - s0) for nm, _, s0, s1 in ev if nm.startswith("k_points_decompress")]
                assert len(mine) == 2
                ms.append(sum(mine))
            say("  K = %-3d %5d points  %9.3f %9.3f %9.3f   %7.3f us per point (median)" %
                (b, b * points, min(ms), statistics.median(ms), max(ms), 1e3 * statistics.median(ms) / (b * points)))
        say()
        for name in ("k_points_decompress", "k_fe_sqrt"):
            for sym, vgpr, agpr, lds, scratch in kernel_figures(_lib.LIB_PATH, name):
                say(f"  {sym}: {vgpr} VGPRs + {agpr} AGPRs, {lds} B LDS, {scratch} B scratch")
        if res:
            say()
            for b in (16, 1):
                if (b, "d") in res:
                    c, d = res[b, "c"], res[b, "d"]
                    say(f"K = {b}: (d)/(c) = {d[1] / c[1]:.3f} by medians; (d) max {d[2]:.3f} {'<' if d[2] < c[0] else '>='} (c) min {c[0]:.3f}: "
                        f"{'faster' if d[2] < c[0] else 'not shown faster'}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    pp.free()
    ctx.close()


if __name__ == "__main__":
    main()
