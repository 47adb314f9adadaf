#!/usr/bin/env python3
"""Measurements of the repeated-rounds seam (vdf_cs_repeat) on one MI355X, profiler off (output: profiles/r13_custom_rounds.txt).

  (1) prove_step_custom of the forward MinRoot round written through the seam, rounds on the device, against the SAME circuit as
      a plain loop of vdf_cs_* calls (every variable made by a host callback, the whole witness uploaded): `--steps` steps at
      t = 2^log2t after a warm-up, three alternations in one process.  Both forms are C callbacks: the runs are those of
      examples/prove_custom_rounds ... bench, a child process started before this one opens the GPU.
      Expectation: the device path beats the plain loop; if it does not the feature is not worth having.
  (2) the same chain under built-in kind 3 (VDF_CIRCUIT_MINROOT_FORWARD), three runs after a warm-up.  Custom circuits keep the
      cross term in one piece (no early rows, no lookahead, no stencil): parity with this rate is NOT expected; the distance is
      reported.
  (3) k_round_tape beside k_forward_segment (the lanes kernel at L = 1) on the same trace, per-launch HIP events, medians.
      How far the interpreter lands from the hand-written kernel is reported, not bounded."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_custom_rounds.txt"))
    a = ap.parse_args()
    t = 1 << a.log2t
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "w")

    def out(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    out("repeated rounds of a custom step circuit, t = 2^%d, %d steps; GPU_MAX_HW_QUEUES = %s" % (
        a.log2t, a.steps, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    # ---- (1) a child process, before this one touches the GPU
    exe = os.path.join(ROOT, "examples", "prove_custom_rounds")
    r = subprocess.run([exe, str(t), str(a.steps), "123", "bench"], capture_output=True, text=True, timeout=1100)
    out("(1) %s %d %d 123 bench -> exit %d" % (os.path.relpath(exe, ROOT), t, a.steps, r.returncode))
    for ln in r.stdout.splitlines():
        out("    " + ln)
    if r.returncode != 0:
        out("    stderr: " + r.stderr[-1000:])
    runs = re.findall(r"repeat on the device ([0-9.]+) ms per step, plain loop ([0-9.]+) ms per step", r.stdout)
    if runs:
        dev_ms, loop_ms = statistics.median(float(x) for x, _ in runs), statistics.median(float(y) for _, y in runs)
        out("    medians: repeat on the device %.4f ms per step, plain loop %.4f ms per step -> %.2fx; the device path %s the plain loop" % (
            dev_ms, loop_ms, loop_ms / dev_ms, "beats" if dev_ms < loop_ms else "DOES NOT beat"))
    # ---- (2) built-in kind 3 over a chain of the same size
    import numpy as np
    import torch
    import vdf_amd
    from vdf_amd.minroot import EvalMode, FIELD_FQ, PallasVDF, State
    from vdf_amd.nova import CIRCUIT_MINROOT_FORWARD, ForwardCircuits, NovaVDFProof, public_params, record_round_body
    ctx = vdf_amd.Context(0)
    vdf = PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential)
    initial = State.from_ints(FIELD_FQ, 123, 0, 0)
    states = vdf.eval_checkpoints(initial, t * a.steps, t)
    pp = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)
    z0, fc = ForwardCircuits.begin(t, initial)
    for k in range(a.steps):
        fc.push_checkpoints(t, states[k:k + 2])
    fc.materialize(ctx)
    ms = []
    for rep in range(4):
        t0 = time.perf_counter()
        p = NovaVDFProof.prove_recursively(pp, fc, t, z0)
        dt = time.perf_counter() - t0
        if rep:
            ms.append(1e3 * dt / a.steps)
        p.free()
    out("(2) built-in kind 3, same chain: %s ms per step, median %.4f" % (" ".join("%.4f" % x for x in ms), statistics.median(ms)))
    if runs:
        out("    repeat on the device / kind 3: %.2fx (custom circuits keep T in one piece: parity is not expected)" % (dev_ms / statistics.median(ms)))
    fc.free(); pp.free()
    # ---- (3) the two kernels on one trace
    from rounds_spec import F
    _, tr = vdf.eval_with_trace(initial, t)
    d_trace = torch.from_numpy(np.ascontiguousarray(tr).view(np.int64)).cuda()
    tape = record_round_body(F(t, "repeat").body())
    i_in = np.frombuffer(initial.i, dtype="<u8").reshape(1, 4).copy()
    seg = torch.zeros((3 * t + 1, 4), dtype=torch.int64, device="cuda")
    ctx.set_kernel_timing(True)
    for _ in range(21):
        ctx.round_tape_run(FIELD_FQ, tape, t, i_in, d_trace, seg)
        ctx.minroot_forward_segment(FIELD_FQ, d_trace, t, i_in, seg)
    ctx.sync()
    ev = ctx.kernel_events()
    for name in ("k_round_tape", "k_forward_segment"):
        d = [e[3] - e[2] for e in ev if e[0] == name][1:]
        out("(3) %-18s %d launches: median %.4f ms, min %.4f, max %.4f" % (name, len(d), statistics.median(d), min(d), max(d)))
    out("    tape of the round: %d ops, %d slots (%d KiB of LDS per workgroup of 64)" % (len(tape.op_list()), tape.c.n_slots, 2 * tape.c.n_slots))
    ctx.close()


if __name__ == "__main__":
    main()
