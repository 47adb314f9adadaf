#!/usr/bin/env python3
"""Measurements of the forward walk (k_forward_walk, vdf_amd/csrc/minroot.hip) on one MI355X, one command (output:
profiles/r08_forward_walk.txt by default).

  (a) rounds per second by n: n = 64, 4,096, 2^16, 2^17, 2^18, 2^19 chains, both fields, `--rounds` rounds (1,024) in launches of
      at most `--launch` rounds, per-launch HIP events (vdf_ctx_set_kernel_timing), one warm-up and `--repeats` timed walks, the
      median.  The n = 64 line is the LATENCY of a lone wavefront: microseconds per round of one chain.
  (b) the yardstick: the host evaluator (vdf_minroot_eval, LTRAddChainSequential) on `--threads` threads (16), each its own
      chain, aggregate rounds per second -- with `--nova-lib PATH` through another build of libvdf_nova.so (the parent
      commit's).  The condition of DESIGN.md 4.8: the device's best aggregate rate is above this one.
  (c) a prover beside a walk: prove_step/s of one prover (t = 2^16, the reference's circuit) alone and while a second thread
      walks 2^17 chains on a second context, alternating; reported, not gated.
  --walk-once N ROUNDS: nothing but one walk of N chains over Fq (after a warm-up launch of one round), for a counter run of
      its own:  rocprofv3 --pmc SQ_INSTS_VALU -- python3 tools/gpu_forward_walk_time.py --walk-once 65536 64
      SQ_INSTS_VALU counts per wavefront: per lane-round = counter / (N / 64 * ROUNDS)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_states(n, seed):
    st = np.random.default_rng(seed).integers(0, 2**64, size=(n, 12), dtype=np.uint64)
    st[:, 3::4] &= np.uint64(0x3FFFFFFFFFFFFFFF)             # below 2^254: canonical Montgomery residues of either field
    return st


def walk_ms(ctx, field, d_states, n, rounds, launch):
    """device milliseconds of one walk of `rounds` rounds cut into launches (sum of the launches' own event spans)"""
    ctx.set_kernel_timing(True)
    done = 0
    while done < rounds:
        now = min(launch, rounds - done)
        ctx.minroot_forward_walk(field, d_states, n, now, base=done)
        done += now
    ev = [e for e in ctx.kernel_events() if e[0] == "k_forward_walk"]
    ctx.set_kernel_timing(False)
    return sum(e[3] - e[2] for e in ev)


def rates(ctx, out, rounds, launch, repeats, sizes):
    import torch
    from vdf_amd.minroot import FIELD_FP, FIELD_FQ
    out("(a) k_forward_walk: %d rounds per walk in launches of <= %d, median of %d after one warm-up" % (rounds, launch, repeats))
    out("    %5s %8s %10s %10s %10s %14s %16s" % ("field", "chains", "ms min", "ms median", "ms max", "us/round/chain", "M rounds/s (all)"))
    best = {}
    for field, name in ((FIELD_FQ, "Fq"), (FIELD_FP, "Fp")):
        for n in sizes:
            d_states = torch.from_numpy(random_states(n, n + field).view(np.int64)).cuda()
            ms = [walk_ms(ctx, field, d_states, n, rounds, launch) for _ in range(repeats + 1)][1:]
            med = statistics.median(ms)
            rate = n * rounds / (med * 1e-3)
            best[name] = max(best.get(name, 0.0), rate)
            out("    %5s %8d %10.3f %10.3f %10.3f %14.2f %16.2f" % (name, n, min(ms), med, max(ms), med * 1e3 / rounds, rate * 1e-6))
            del d_states
            torch.cuda.empty_cache()
    return best


def host_yardstick(out, threads, rounds, nova_lib_path):
    from vdf_amd.minroot import FIELD_FP, FIELD_FQ, _State, nova_lib
    lib = nova_lib
    if nova_lib_path:
        lib = C.CDLL(nova_lib_path)
        lib.vdf_minroot_eval.argtypes = nova_lib.vdf_minroot_eval.argtypes
        lib.vdf_minroot_eval.restype = C.c_int
    out("(b) host evaluator, %d threads x %d rounds each, LTRAddChainSequential%s" % (threads, rounds, " through " + nova_lib_path if nova_lib_path else ""))
    res = {}
    for field, name in ((FIELD_FQ, "Fq"), (FIELD_FP, "Fp")):
        st = random_states(threads, 9 + field)
        spans = []
        for _ in range(3):
            outs = [_State() for _ in range(threads)]
            ins = [_State.from_buffer_copy(st[k].tobytes()) for k in range(threads)]
            ths = [threading.Thread(target=lambda k=k: lib.vdf_minroot_eval(field, 1, C.byref(ins[k]), rounds, C.byref(outs[k]), None)) for k in range(threads)]
            a = time.perf_counter()
            for th in ths: th.start()
            for th in ths: th.join()
            spans.append(time.perf_counter() - a)
        t = statistics.median(spans)
        res[name] = threads * rounds / t
        out("    %5s %8.3f s  -> %8.2f M rounds/s aggregate, %6.2f us per round per thread" % (name, t, res[name] * 1e-6, t * 1e6 / rounds))
    return res


def prover_beside(ctx, out, steps, launch):
    import torch
    import vdf_amd
    from vdf_amd.minroot import PallasVDF, State, FIELD_FQ, EvalMode
    from vdf_amd.nova import InverseMinRootCircuit, NovaVDFProof, public_params
    t, n_walk = 1 << 16, 1 << 17
    out("(c) one prover (t = 2^16, %d steps, steps 2.. timed) alone and beside a walk of 2^17 chains in launches of %d rounds on a second context" % (steps, launch))
    initial = State.from_ints(FIELD_FQ, 0x1234567890ABCDEF, 0, 0)
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential), t, steps, initial)
    pp = public_params(ctx, t)
    circuits.upload(ctx)
    side = vdf_amd.Context(0)
    d_states = torch.from_numpy(random_states(n_walk, 3).view(np.int64)).cuda()

    def prove():
        proof = NovaVDFProof.prove_step(pp, None, circuits, 0, z0)
        proof = NovaVDFProof.prove_step(pp, proof, circuits, 1, z0)
        ctx.sync()
        a = time.perf_counter()
        for k in range(2, steps):
            proof = NovaVDFProof.prove_step(pp, proof, circuits, k, z0)
        ctx.sync()
        b = time.perf_counter()
        wire = proof.serialize()
        proof.free()
        return (steps - 2) / (b - a), wire
    prove()
    solo, beside, wires, walked = [], [], set(), []
    for _ in range(3):
        r, w = prove()
        solo.append(r); wires.add(w)
        stop, count = threading.Event(), [0]

        def walker():
            while not stop.is_set():
                side.minroot_forward_walk(FIELD_FQ, d_states, n_walk, launch)
                count[0] += 1
        th = threading.Thread(target=walker)
        a = time.perf_counter()
        th.start()
        r, w = prove()
        stop.set()
        th.join()
        walked.append(count[0] * n_walk * launch / (time.perf_counter() - a))
        beside.append(r); wires.add(w)
    out("    prove_step/s alone  %s (median %.1f)" % (" ".join("%.1f" % v for v in solo), statistics.median(solo)))
    out("    prove_step/s beside %s (median %.1f); the walker meanwhile: %.1f M rounds/s; proofs identical: %s" %
        (" ".join("%.1f" % v for v in beside), statistics.median(beside), statistics.median(walked) * 1e-6, len(wires) == 1))
    side.close()
    circuits.free(); pp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_forward_walk.txt"))
    ap.add_argument("--rounds", type=int, default=1024)
    ap.add_argument("--launch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-rounds", type=int, default=1 << 16)
    ap.add_argument("--nova-lib", default="")
    ap.add_argument("--sizes", default="64,4096,65536,131072,262144,524288")
    ap.add_argument("--prover-steps", type=int, default=12)
    ap.add_argument("--no-prover", action="store_true")
    ap.add_argument("--walk-once", nargs=2, type=int, metavar=("N", "ROUNDS"))
    args = ap.parse_args()
    import torch
    import vdf_amd
    from vdf_amd import _lib
    from vdf_amd.minroot import FIELD_FQ
    ctx = vdf_amd.Context(0)
    launch = min(args.launch, _lib.MINROOT_FORWARD_MAX_ROUNDS)
    if args.walk_once:
        n, rounds = args.walk_once
        d_states = torch.from_numpy(random_states(n, 1).view(np.int64)).cuda()
        ctx.minroot_forward_walk(FIELD_FQ, d_states, n, 1)
        ctx.minroot_forward_walk(FIELD_FQ, d_states, n, rounds)
        print("walked %d chains x %d rounds (+ 1 warm-up round): %d wavefront-rounds" % (n, rounds, (n + 63) // 64 * rounds))
        ctx.close()
        return
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("tools/gpu_forward_walk_time.py on %s; VDF_MINROOT_FORWARD_MAX_ROUNDS = %d" % (torch.cuda.get_device_name(0), _lib.MINROOT_FORWARD_MAX_ROUNDS))
    best = rates(ctx, out, args.rounds, launch, args.repeats, [int(v) for v in args.sizes.split(",")])
    host = host_yardstick(out, args.threads, args.host_rounds, args.nova_lib)
    for name in ("Fq", "Fp"):
        out("    %s: device best %.2f M rounds/s = %.1f x the host's %d threads (%.2f M rounds/s): condition %s" %
            (name, best[name] * 1e-6, best[name] / host[name], args.threads, host[name] * 1e-6, "MET" if best[name] > host[name] else "NOT MET"))
    if not args.no_prover:
        prover_beside(ctx, out, args.prover_steps, launch)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
