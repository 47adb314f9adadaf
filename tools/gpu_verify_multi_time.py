"""The batch verifier of compressed proofs with every proof's M(r_x, r_y) in passes over the shape (vdf_nova_pp_set_verify_multi)
against the per-proof sequence, at t = 2^16: 16 proofs of distinct chains in one process, batches of K = 1, 2, 4, 8, 16, the two
modes (n = 0 and n = --points) taking turns repeat by repeat; per K and mode the minimum, median and maximum ms per proof.  Then,
from the HIP events the library puts around its launches, one batch of 16 in each mode: the new kernel's own time
(k_sparse_eval_multi, both launches) and the eq tables it needs, against the old sequence's replay kernels (eq tables, k_spmvt
with its heavy columns, the dot) for the same points; and the kernel's registers, LDS and waves per SIMD from the library's code
object.  The last lines state the rule for the default and what this run says.

The baseline is never the code under test: run the same file on a built checkout of the parent commit with --root (it then has
no switch and times the batch verifier as that commit has it), in the same session, and keep the two records side by side:
  python tools/gpu_verify_multi_time.py --root /path/to/parent/checkout --out parent.txt
  python tools/gpu_verify_multi_time.py --out profiles/rNN_verify_multi.txt
A build with four instances per pass (make ab AB_FLAGS=-DVDF_SPARSE_EVAL_CHUNK=4) is timed with VDF_HIP_LIB set to it.
usage: python tools/gpu_verify_multi_time.py [--lg 16] [--proofs 16] [--repeats 5] [--points 16] [--root DIR] [--out FILE]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_REPLAY = ("k_eq_table", "k_spmvt", "k_reduce")
NEW_KERNEL = "k_sparse_eval_multi"
LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def kernel_figures(lib_path, name):
    """[(symbol, VGPRs, AGPRs, LDS bytes, scratch bytes)] of the kernels whose name contains `name`, from the gfx950 code object"""
    run = lambda tool, *args: subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
        run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib_path, os.path.join(tmp, "copy"))
        blob, magic = open(fat, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(magic, blob)]              # one bundle per translation unit, back to back
        for lo, hi in zip(starts, starts[1:] + [len(blob)]):
            with open(fat, "wb") as f:
                f.write(blob[lo:hi])
            run("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co)
            if not os.path.getsize(co):
                continue
            cur = None
            for line in run("llvm-readelf", "--notes", co).splitlines() + ["  - .end: x"]:
                m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(.*)$", line)
                if not m:
                    continue
                if m.group(1) == "  - ":
                    if cur and name in cur.get(".name", ""):
                        out.append(cur)
                    cur = {}
                if cur is not None:
                    cur[m.group(2)] = m.group(3).strip().strip("'")
    return [(k[".name"], int(k[".vgpr_count"]), int(k.get(".agpr_count", 0)), int(k[".group_segment_fixed_size"]),
             int(k[".private_segment_fixed_size"])) for k in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--points", type=int, default=16)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import vdf_amd
    from oracle import pasta as o
    from vdf_amd import _lib
    from vdf_amd.minroot import PallasVDF, State, FIELD_FQ
    from vdf_amd.nova import InverseMinRootCircuit, NovaVDFProof, public_params, verify_compressed_batch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t, P = 1 << a.lg, a.proofs
    ctx = vdf_amd.Context(0)
    pp = public_params(ctx, t)
    has_switch = hasattr(pp, "set_verify_multi")
    modes = [0, a.points] if has_switch else [None]
    name = {0: "n = 0 (per proof)", a.points: f"n = {a.points} (passes)", None: "no switch (baseline)"}
    items = []
    t0 = time.perf_counter()
    for q in range(P):
        x = o.rand_fe(7000 + q, 0, o.Q)
        init = State.from_ints(FIELD_FQ, x, 0, 1)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, a.steps, init)
        snark = NovaVDFProof.prove_recursively(pp, circuits, t, z0).compress(pp)
        items.append((snark, a.steps, z0, [init.x, init.y, init.i]))
    say(f"library {os.path.relpath(_lib.LIB_PATH, os.path.abspath(a.root))} of {'this checkout' if os.path.abspath(a.root) == HERE else 'the checkout given with --root'}")
    say(f"t = 2^{a.lg}: {P} compressed proofs of distinct chains ({a.steps} steps each) made in {time.perf_counter() - t0:.1f} s; "
        f"{a.repeats} repeats per figure, the modes taking turns; ms per proof")

    def set_mode(n):
        if n is not None:
            pp.set_verify_multi(n)

    for n in modes:                                                  # warm-up of every shape and allocation the timed window uses
        set_mode(n)
        assert verify_compressed_batch(pp, items) == [True] * P
    res = {}
    say("  %-4s %-22s %9s %9s %9s" % ("K", "mode", "min", "median", "max"))
    for b in (1, 2, 4, 8, 16):
        if b > P:
            break
        reps = {n: [] for n in modes}
        for _ in range(a.repeats):
            for n in modes:
                set_mode(n)
                ctx.sync()
                t0 = time.perf_counter()
                got = verify_compressed_batch(pp, items[:b])
                reps[n].append((time.perf_counter() - t0) * 1e3 / b)
                assert got == [True] * b
        for n in modes:
            res[b, n] = (min(reps[n]), statistics.median(reps[n]), max(reps[n]))
            say("  %-4d %-22s %9.3f %9.3f %9.3f" % ((b, name[n]) + res[b, n]))

    for n in modes:
        set_mode(n)
        ctx.sync()
        ctx.set_kernel_timing(True)
        ctx.kernel_events()
        t0 = time.perf_counter()
        assert verify_compressed_batch(pp, items) == [True] * P
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ev = ctx.kernel_events()
        ctx.set_kernel_timing(False)
        ms = lambda pred: sum(s1 - s0 for nm, _, s0, s1 in ev if pred(nm))
        count = lambda pred: sum(1 for nm, *_ in ev if pred(nm))
        busy = ms(lambda nm: True)
        say()
        say(f"one batch of {P}, {name[n]}: {wall:.2f} ms with events on; launches timed {len(ev)}, device busy {busy:.2f} ms, "
            f"host work, copies and waits {wall - busy:.2f} ms")
        is_old = lambda nm: nm.startswith(OLD_REPLAY)
        is_new = lambda nm: nm.startswith(NEW_KERNEL[:23])
        say("  %-58s %4d launches %9.3f ms" % ("eq tables, k_spmvt (+heavy cols), dot", count(is_old), ms(is_old)))
        say("  %-58s %4d launches %9.3f ms" % (NEW_KERNEL + " (with k_sparse_eval_sum)", count(is_new), ms(is_new)))
        if n:
            say("  passes, points, failed since the set was made: %s" % (pp.verify_multi_stats(),))
    if has_switch:
        say()
        for sym, vgpr, agpr, lds, scratch in kernel_figures(_lib.LIB_PATH, "k_sparse_eval"):
            regs = (vgpr + 7) // 8 * 8 + (agpr + 7) // 8 * 8
            say(f"  {sym}: {vgpr} VGPRs + {agpr} AGPRs, {lds} B LDS, {scratch} B scratch, {min(8, 512 // max(regs, 1))} waves per SIMD by registers")
        top, one = min(16, P), 1
        if (top, 0) in res and (one, 0) in res:
            a16 = res[top, a.points][2] < res[top, 0][0]
            a1 = res[one, a.points][1] <= res[one, 0][2]
            say()
            say(f"rule for the default: n = {a.points} when at K = {top} its maximum lies below the old mode's minimum "
                f"({res[top, a.points][2]:.3f} vs {res[top, 0][0]:.3f}: {'yes' if a16 else 'no'}) and at K = 1 its median lies inside the old "
                f"mode's spread or below it ({res[one, a.points][1]:.3f} vs {res[one, 0][0]:.3f}..{res[one, 0][2]:.3f}: {'yes' if a1 else 'no'})"
                f" -> {a.points if a16 and a1 else 0}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for s, *_ in items:
        s.free()
    pp.free()
    ctx.close()


if __name__ == "__main__":
    main()
