"""Batch verification of running proofs at t = 2^16 (profiles/r06_verify_running_batch.txt): 16 running proofs of distinct
chains (1 or 2 steps) in one process; the single verifier over all 16 against vdf_nova_verify_batch over the first 1, 2, 4, 8
and 16, five repeats each, median ms per proof; then where the time of one batch of 16 (and of one single verification) goes,
from the HIP events the library puts around its launches: per side the linear combination of the witnesses
(k_lincomb_u128, with its achieved bandwidth), the MSM over the generators, the MSM over the commitments, the combined residual
(k_relaxed_residual_batch) -- or, for the single verifier, its five MSMs and its sparse and residual kernels.
usage: python tools/gpu_verify_running_batch_time.py [--lg 16] [--proofs 16] [--repeats 5] [--out FILE] [--rev COMMIT]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vdf_amd  # noqa: E402
from oracle import pasta as o  # noqa: E402
from vdf_amd.minroot import PallasVDF, State, FIELD_FQ  # noqa: E402
from vdf_amd.nova import InverseMinRootCircuit, NovaVDFProof, public_params, verify_batch  # noqa: E402

MSM_START = ("k_glv_split", "msm_sort", "k_direct_sum")
MSM_ANY = MSM_START + ("k_accumulate", "msm_tail", "msm_fixup", "k_direct_final")
GEN_MSM_MIN = 1 << 13            # an MSM over at least this many entries is one over the generators (the commitments: 2K or 3K)


def split(events, per_side=True):
    """{phase: [device ms, algorithmic bytes]} of a drained event list (launches in time order); per_side: a batch's launches,
    whose k_lincomb_u128 opens side 0 and side 1."""
    out = {}
    side, msm, last = -1, None, ""

    def add(key, ms, nbytes=0.0):
        v = out.setdefault(key, [0.0, 0.0])
        v[0] += ms
        v[1] += nbytes
    for name, nbytes, s0, s1 in sorted(events, key=lambda e: e[2]):
        ms = s1 - s0
        if name.startswith(MSM_ANY):
            starts = name.startswith(MSM_START) and not (name.startswith("msm_sort") and last.startswith("k_glv_split"))
            if starts or msm is None:
                msm = {"n": 0, "ms": 0.0, "side": side}
                out.setdefault("_msms", []).append(msm)
            if nbytes:
                msm["n"] = max(msm["n"], int(nbytes / 96))
            msm["ms"] += ms
            last = name
            continue
        if name == "k_lincomb_u128":
            if per_side and not last.startswith("k_lincomb"):
                side += 1
            add(f"k_lincomb_u128, side {side}" if per_side else name, ms, nbytes)
        elif name.startswith("k_relaxed_residual"):             # (event names keep 23 characters)
            add(f"k_relaxed_residual_batch, side {side}" if per_side else name, ms, nbytes)
        else:
            add("other: " + name, ms, nbytes)
        msm, last = None, name
    for m in out.pop("_msms", []):
        kind = "generator MSM" if m["n"] >= GEN_MSM_MIN else "commitment MSM"
        add(f"{kind}, side {m['side']}" if per_side else f"{kind}s", m["ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rev", default=None, help="the commit to name in the output (default: git rev-parse HEAD)")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rev = a.rev
    try:
        rev = rev or subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], text=True,
                                      cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))).strip()
    except Exception:
        rev = "unknown"
    t, P = 1 << a.lg, a.proofs
    ctx = vdf_amd.Context(0)
    pp = public_params(ctx, t)
    items = []
    t0 = time.perf_counter()
    for q in range(P):
        x = o.rand_fe(9000 + q, 0, o.Q)
        init = State.from_ints(FIELD_FQ, x, 0, 1)
        steps = 1 + q % 2
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, steps, init)
        items.append((NovaVDFProof.prove_recursively(pp, circuits, t, z0), steps, z0, [init.x, init.y, init.i]))
    say(f"commit {rev}; t = 2^{a.lg}: {P} running proofs of distinct chains (1-2 steps) made in {time.perf_counter() - t0:.1f} s; "
        f"{a.repeats} repeats per figure, median ms per proof")
    assert all(p.verify(pp, n, z0, zi) for p, n, z0, zi in items)
    assert verify_batch(pp, items) == [True] * P                     # warm-up of every shape the timed window uses

    def timed(fn, per):
        reps = []
        for _ in range(a.repeats):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            reps.append((time.perf_counter() - t0) * 1e3 / per)
        return statistics.median(reps), min(reps), max(reps)

    def single_all():
        assert all(p.verify(pp, n, z0, zi) for p, n, z0, zi in items)

    med, lo, hi = timed(single_all, P)
    single = med
    say(f"single verifier x{P:<3d}        {med:8.2f} ms/proof  (range {lo:.2f}-{hi:.2f})")
    for b in (1, 2, 4, 8, 16):
        if b > P:
            break
        med, lo, hi = timed(lambda: verify_batch(pp, items[:b]), b)
        say(f"batch verifier, {b:2d} proofs    {med:8.2f} ms/proof  (range {lo:.2f}-{hi:.2f})  {med / single:5.2f} x single")

    for label, fn, per, per_side in (("one batch of %d" % P, lambda: verify_batch(pp, items), P, True),
                                     ("one single verification", lambda: items[0][0].verify(pp, *items[0][1:]), 1, False)):
        ctx.sync()
        ctx.set_kernel_timing(True)
        ctx.kernel_events()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ev = ctx.kernel_events()
        ctx.set_kernel_timing(False)
        ph = split(ev, per_side)
        dev = sum(v[0] for v in ph.values())
        say()
        say(f"{label}: {wall:.2f} ms with events on ({wall / per:.2f} ms/proof); launches {len(ev)}, device busy {dev:.2f} ms, "
            f"host work, copies and waits {wall - dev:.2f} ms")
        say("  %-46s %9s %12s %14s" % ("phase (device time of its launches)", "ms", "ms/proof", "TB/s (of 8)"))
        for k, (ms, nbytes) in sorted(ph.items(), key=lambda kv: -kv[1][0]):
            bw = "%14.2f" % (nbytes / ms / 1e9) if nbytes and ms > 0 else ""
            say("  %-46s %9.3f %12.3f %s" % (k, ms, ms / per, bw))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    pp.free()
    ctx.close()


if __name__ == "__main__":
    main()
