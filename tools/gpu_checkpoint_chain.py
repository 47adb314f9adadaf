#!/usr/bin/env python3
"""Measurements of the checkpoint path on one MI355X, one command (output: profiles/r06_checkpoint_chain.txt by default).

  (a) k_inverse_walk alone: per-launch HIP events (vdf_ctx_set_kernel_timing), one warm-up and `--repeats` timed launches of
      2^16-round walks for n = 1, 64, 256, 4,096, 65,536 and of 256 x 64 walks of 2^10 rounds: ns per round (a lane's), walks
      per second, GB/s written.  A trace is written where it fits 32 GiB (n <= 4,096 at 2^16 rounds); n = 65,536 walks without.
  (b) the prover: prove_step/s over a chain of `--steps` steps at t = 2^16 (the reference's circuit) in ONE process, alternating
      `--repeats` times between (i) traces resident up front -- today's path -- and (ii) checkpoint circuits (every = t) through
      the windowed prove_recursively, window 0 materialised before the clock starts as (i)'s upload is.  (ii-cold) is the same
      with nothing resident: the first window's walk is inside the clock.  Device bytes of the traces and the process's peak
      RSS are recorded; then fresh child processes run (ii) alone with other launch bounds (VDF_NOVA_WALK_LAUNCH), windows and
      with every < t, and report their own peak RSS: a prover that never held a trace.
The forward evaluation that feeds both (about 0.35 s per step on the host) is set-up, outside every timed region.
Each child runs under its own time limit and the first failure ends the run."""
import argparse
import json
import os
import resource
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rss_mb():
    """peak resident set of THIS process image (VmHWM; ru_maxrss survives fork and exec and would report the parent's)"""
    for ln in open("/proc/self/status"):
        if ln.startswith("VmHWM:"):
            return int(ln.split()[1]) / 1024.0
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def kernel_alone(ctx, out, repeats):
    import torch
    from vdf_amd.minroot import FIELD_FQ
    from oracle import pasta as o
    out("(a) k_inverse_walk alone; estimate from DESIGN.md 4.1: ~1,200 ns per round, 2^16 rounds ~ 80 ms whatever n is while waves do not share a SIMD")
    out("    %8s %8s %6s %10s %10s %10s %12s %12s %10s" % ("walks", "rounds", "trace", "ms min", "ms median", "ms max", "ns/round", "walks/s", "GB/s"))
    rng = np.random.default_rng(5)
    for n, rounds, group in ((1, 1 << 16, 0), (64, 1 << 16, 0), (256, 1 << 16, 0), (4096, 1 << 16, 0), (65536, 1 << 16, 0), (256 * 64, 1 << 10, 64)):
        with_trace = n * rounds * 64 <= (32 << 30)
        st = rng.integers(0, 2**64, size=(n, 12), dtype=np.uint64)
        st[:, 3::4] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        d_states = torch.from_numpy(st.view(np.int64)).cuda()
        if with_trace:
            per_group = (group or 1) * rounds + 1
            d_trace = torch.empty(((n // (group or 1)) * per_group * 8,), dtype=torch.int64, device="cuda")
        ms = []
        for rep in range(repeats + 1):
            ctx.set_kernel_timing(True)
            if not with_trace:
                ctx.minroot_inverse_walk(FIELD_FQ, d_states, n, rounds)
            elif group:
                ctx.minroot_inverse_walk(FIELD_FQ, d_states, n, rounds, d_trace, walk_stride=rounds, top=rounds, group=group, group_stride=per_group)
            else:
                ctx.minroot_inverse_walk(FIELD_FQ, d_states, n, rounds, d_trace, walk_stride=rounds + 1, top=rounds)
            ev = [e for e in ctx.kernel_events() if e[0] == "k_inverse_walk"]
            ctx.set_kernel_timing(False)
            if rep:
                ms.append(ev[0][3] - ev[0][2])
        med = statistics.median(ms)
        out("    %8d %8d %6s %10.3f %10.3f %10.3f %12.1f %12.1f %10.2f" % (n, rounds, "yes" if with_trace else "no", min(ms), med, max(ms),
                                                                   med * 1e6 / rounds, n / (med * 1e-3), (n * rounds * 64 / (med * 1e-3) / 1e9) if with_trace else 0.0))
        del d_states
        if with_trace:
            del d_trace
        torch.cuda.empty_cache()


def timed_prove(pp, circuits, t, z0, window, ctx):
    from vdf_amd.nova import NovaVDFProof
    import gc
    gc.collect()
    gc.disable()
    a = time.perf_counter()
    proof = NovaVDFProof.prove_recursively(pp, circuits, t, z0, window_steps=window)
    ctx.sync()
    s = time.perf_counter() - a
    gc.enable()
    return proof, s


def checkpoint_runs(ctx, pp, t, n, states, every, window, repeats, out, label, want=None, cold=False):
    """`repeats` runs of the windowed prove_recursively over fresh checkpoint circuits; returns the steps/s of each"""
    from vdf_amd.nova import InverseMinRootCircuit
    rates, peak = [], 0
    for _ in range(repeats):
        z0, cc = InverseMinRootCircuit.from_checkpoints(t, every, n, states)
        w = window or max(2, (1 << 30) // ((t + 1) * 64))
        if not cold:
            cc.materialize(ctx, 0, min(w, n))
        proof, s = timed_prove(pp, cc, t, z0, window, ctx)
        cc.release()
        if want is not None and proof.serialize() != want:
            raise SystemExit("the proof over checkpoint circuits differs from the proof over resident traces")
        rates.append(n / s)
        proof.free(); cc.free()
    out("    %-44s %s   median %.1f  min %.1f  max %.1f prove_step/s" % (label, " ".join("%.1f" % r for r in rates), statistics.median(rates), min(rates), max(rates)))
    return rates


def child(args):
    """(ii) alone in a fresh process: checkpoint states from the file, never a trace on the host"""
    import vdf_amd
    from vdf_amd.minroot import State
    from vdf_amd.nova import public_params
    raw = np.load(args.child).tobytes()
    states = [State(raw[96 * k:96 * k + 32], raw[96 * k + 32:96 * k + 64], raw[96 * k + 64:96 * k + 96]) for k in range(len(raw) // 96)]
    t = 1 << args.log2t
    every = 1 << args.log2every
    n = (len(states) - 1) // (t // every)
    ctx = vdf_amd.Context(0)
    ctx.set_async(True)
    pp = public_params(ctx, t)
    lines = []
    checkpoint_runs(ctx, pp, t, n, states, every, args.window, 1, lambda s: None, "warm-up")
    checkpoint_runs(ctx, pp, t, n, states, every, args.window, args.repeats, lines.append,
                    "(ii) every=2^%d window=%s launch=%s" % (args.log2every, args.window or "1GiB", os.environ.get("VDF_NOVA_WALK_LAUNCH", "1024")))
    print(lines[0] + "   peak RSS %.0f MB" % rss_mb())
    pp.free(); ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_checkpoint_chain.txt"))
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--log2t", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=int, default=0, help="steps per window of (ii); 0 = the library's default (1 GiB of traces)")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-children", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--log2every", type=int, default=16, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import vdf_amd
    from vdf_amd.minroot import EvalMode, PallasVDF, State, FIELD_FQ
    from vdf_amd.nova import InverseMinRootCircuit, public_params
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def out(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    out("checkpoint chain: GPU_MAX_HW_QUEUES=%s, VDF_NOVA_WALK_LAUNCH=%s" % (
        os.environ.get("GPU_MAX_HW_QUEUES", "unset"), os.environ.get("VDF_NOVA_WALK_LAUNCH", "unset (1024)")))
    ctx = vdf_amd.Context(0)
    if not args.no_kernel:
        kernel_alone(ctx, out, args.repeats)
    t, n = 1 << args.log2t, args.steps
    initial = State.from_ints(FIELD_FQ, 0x1234567890ABCDEF1234567890ABCDEF, 0, 0)
    vdf = PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential)
    a = time.perf_counter()
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(vdf, t, n, initial)
    out("(b) %d steps at t = 2^%d; forward evaluation (set-up, host): %.1f s; peak RSS with the traces on the host %.0f MB" % (n, args.log2t, time.perf_counter() - a, rss_mb()))
    states = [circuits.states(n - 1)[1]] + [circuits.states(n - 1 - s)[0] for s in range(n)]
    pp = public_params(ctx, t)
    ctx.set_async(True)
    circuits.upload(ctx)
    out("    (i) traces resident: %d steps, %d bytes of HBM; (ii) at most two windows of %d steps: %d bytes" % (
        n, n * (t + 1) * 64, args.window or max(2, (1 << 30) // ((t + 1) * 64)), 2 * min(n, args.window or max(2, (1 << 30) // ((t + 1) * 64))) * (t + 1) * 64))
    # the states every 2^10 rounds, for the children that measure every < t: read out of the resident traces (a second forward
    # evaluation would be three more minutes of set-up); i counts rounds from the initial state's 0
    from vdf_amd._lib import lib
    fine = {1 << 10: [states[0]]}
    buf = np.zeros((t + 1, 8), dtype="<u8")
    for s_ in range(n):
        assert lib.vdf_dev_memcpy(ctx.handle, buf.ctypes.data, circuits.trace_ptr(n - 1 - s_), (t + 1) * 64) == 0
        for k in range(1 << 10, t + 1, 1 << 10):
            fine[1 << 10].append(State(buf[k, :4].tobytes(), buf[k, 4:].tobytes(), vdf.element(s_ * t + k)))
    proof, _ = timed_prove(pp, circuits, t, z0, None, ctx)          # settle: clocks, workspaces, helper threads
    want = proof.serialize()
    proof.free()
    checkpoint_runs(ctx, pp, t, n, states, t, args.window, 1, lambda s: None, "warm-up", want)
    ri, rii = [], []
    for rep in range(args.repeats):
        proof, s = timed_prove(pp, circuits, t, z0, None, ctx)
        proof.free()
        ri.append(n / s)
        rii += checkpoint_runs(ctx, pp, t, n, states, t, args.window, 1, lambda s: None, "", want)
    out("    %-44s %s   median %.1f  min %.1f  max %.1f prove_step/s" % ("(i) traces resident (today's path)", " ".join("%.1f" % r for r in ri), statistics.median(ri), min(ri), max(ri)))
    out("    %-44s %s   median %.1f  min %.1f  max %.1f prove_step/s" % ("(ii) checkpoints, windowed, alternating", " ".join("%.1f" % r for r in rii), statistics.median(rii), min(rii), max(rii)))
    out("    margin: (ii) median %.1f against (i) lowest run %.1f: %s" % (statistics.median(rii), min(ri), "holds" if statistics.median(rii) >= min(ri) else "SHORT by %.1f %%" % (100 * (1 - statistics.median(rii) / min(ri)))))
    checkpoint_runs(ctx, pp, t, n, states, t, args.window, args.repeats, out, "(ii-cold) first window inside the clock", want, cold=True)
    circuits.free(); pp.free(); ctx.close()
    if args.no_children:
        return
    # fresh processes: (ii) alone, other launch bounds / windows / every < t
    tmp = tempfile.mkdtemp()
    try:
        for log2e in (args.log2t, 10):
            every = 1 << log2e
            sts = states if every == t else fine[every]
            path = os.path.join(tmp, "states_%d.npy" % log2e)
            np.save(path, np.frombuffer(b"".join(s.x + s.y + s.i for s in sts), dtype="<u8"))
        for log2e, window, launch in ((args.log2t, 0, 1024), (args.log2t, 0, 256), (args.log2t, 0, 8192), (args.log2t, 128, 1024), (10, 0, 1024), (10, 64, 1024)):
            env = dict(os.environ, VDF_NOVA_WALK_LAUNCH=str(launch))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, "states_%d.npy" % log2e), "--log2t", str(args.log2t),
                                "--log2every", str(log2e), "--window", str(window), "--repeats", str(args.repeats)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                out("    child (every 2^%d, window %d, launch %d) failed with %d: %s" % (log2e, window, launch, r.returncode, r.stderr[-1500:]))
                raise SystemExit(1)
            out(r.stdout.rstrip().splitlines()[-1])
    finally:
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    log.close()


if __name__ == "__main__":
    main()
