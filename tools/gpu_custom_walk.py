#!/usr/bin/env python3
"""Measurements of walk tapes (vdf_round_tape_walk, k_tape_walk) on one MI355X, profiler off (output: profiles/r14_custom_walk.txt).
One process, t = 2^log2t rounds per step, `--walks` checkpoint intervals per step.  The chain is made backwards (the inverse round
is cheap), so the tool spends no minutes on fifth roots it does not measure.

  (1) k_tape_walk running the MinRoot inverse round as a tape beside k_inverse_walk, the hand-written kernel, on the same walks:
      per-launch HIP events, medians, and the time per round (a lane's rounds are sequential, the lanes run side by side).
      The yardstick is k_inverse_walk's 1.42 us per round of profiles/r06_checkpoint_chain.txt.  How far the interpreter lands
      from the hand-written walk is reported, not bounded.
  (2) what one step's advice costs either way: walk + k_round_tape (events) against host evaluation of the step
      (vdf_minroot_eval with its trace) + vdf_dev_memcpy of the trace, as examples/prove_custom_rounds.c does it.
  (3) the prove_step_custom rate over `--steps` steps after a warm-up, both ways: advice by one walk launch per step from
      checkpoints in device memory, against a host trace uploaded every step (the trace is made beforehand: the evaluation's own
      cost is (2)'s).  Median of `--runs` alternating runs with the spread."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=16)
    ap.add_argument("--walks", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_custom_walk.txt"))
    a = ap.parse_args()
    t, per = 1 << a.log2t, a.walks
    every = t // per
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "w")

    def out(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    import numpy as np
    import torch
    import vdf_amd
    from vdf_amd._lib import lib
    from vdf_amd.minroot import EvalMode, FIELD_FQ, PallasVDF, State
    from vdf_amd.nova import NovaVDFProof, public_params_custom, record_round_body, record_walk_body, walk_tape_eval
    from rounds_spec import F
    from walks_spec import minroot_body
    from util import dev, states_array
    out("walk tapes, t = 2^%d, %d walks of %d rounds per step, %d steps; GPU_MAX_HW_QUEUES = %s" % (
        a.log2t, per, every, a.steps, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    # the chain, backwards from an arbitrary last state: one checkpoint per interval
    n_cp = a.steps * per
    cps = [State.from_ints(FIELD_FQ, 0x123456789ABCDEF, 0xFEDCBA987654321, 7 + a.steps * t)]
    for _ in range(n_cp):
        cps.insert(0, PallasVDF.inverse_eval(cps[0], every))
    arr = states_array(cps)
    xy, i0 = np.ascontiguousarray(arr[:, :8]), np.ascontiguousarray(arr[0, 8:12]).reshape(1, 4)
    z0 = [cps[0].x, cps[0].y, cps[0].i]
    zi = [cps[-1].x, cps[-1].y, cps[-1].i]
    walk_tape, round_tape = record_walk_body(minroot_body(FIELD_FQ)), record_round_body(F(t, "repeat").body())
    products = sum(op in (6, 7) for op, *_ in walk_tape.op_list())
    out("walk tape: %d ops (%d products), %d slots + 2 x %d columns = %d KiB of LDS per wavefront" % (
        len(walk_tape.op_list()), products, walk_tape.c.n_slots, walk_tape.c.n_adv, 2 * (walk_tape.c.n_slots + 2 * walk_tape.c.n_adv)))
    d_starts = [dev(xy[g * per + 1:g * per + per + 1]) for g in range(a.steps)]       # checkpoints in device memory, per step
    d_expect = [dev(xy[g * per:g * per + per]) for g in range(a.steps)]
    d_trace = torch.zeros((2 * (t + 1), 4), dtype=torch.int64, device="cuda")
    d_ok = torch.zeros(per, dtype=torch.int32, device="cuda")

    def walk_step(g):
        """step g's trace into d_trace from its checkpoints (the walks overwrite their entries: a copy is walked)"""
        st = d_starts[g].clone()
        ctx.round_tape_walk(FIELD_FQ, walk_tape, i0, st, per, every, d_trace, walk_stride=every, top=every, group=per, group_stride=t + 1,
                            j_base=g * t, heads=True, expect=d_expect[g], ok=d_ok)
    # ---- (1) the two kernels on the same walks
    ctx.set_kernel_timing(True)
    d_states = dev(np.ascontiguousarray(arr[1:per + 1]))
    for _ in range(6):
        walk_step(0)
        st = d_states.clone()
        ctx.minroot_inverse_walk(FIELD_FQ, st, per, every, d_trace, walk_stride=every, top=every)
    ctx.sync()
    assert d_ok.cpu().tolist() == [1] * per, "a walk missed its checkpoint"
    ev = ctx.kernel_events()
    med = {}
    for name in ("k_tape_walk", "k_inverse_walk"):
        d = [e[3] - e[2] for e in ev if e[0] == name][1:]
        med[name] = statistics.median(d)
        out("(1) %-15s %d launches of %d walks x %d rounds: median %.3f ms, min %.3f, max %.3f -> %.3f us per round" % (
            name, len(d), per, every, med[name], min(d), max(d), 1e3 * med[name] / every))
    out("    interpreter / hand-written walk: %.2fx (yardstick: 1.42 us per round, profiles/r06_checkpoint_chain.txt)" % (
        med["k_tape_walk"] / med["k_inverse_walk"]))
    # ---- (2) one step's advice, either way
    seg = torch.zeros((3 * t, 4), dtype=torch.int64, device="cuda")
    for _ in range(6):
        walk_step(0)
        ctx.round_tape_run(FIELD_FQ, round_tape, t, i0, d_trace, seg)
    ctx.sync()
    ev = ctx.kernel_events()
    ctx.set_kernel_timing(False)
    w_ms = statistics.median([e[3] - e[2] for e in ev if e[0] == "k_tape_walk"][1:])
    r_ms = statistics.median([e[3] - e[2] for e in ev if e[0] == "k_round_tape"][1:])
    vdf = PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential)
    ev_ms, cp_ms, tr = [], [], None
    for _ in range(3):
        t0 = time.perf_counter()
        _, tr = vdf.eval_with_trace(cps[0], t)
        ev_ms.append(1e3 * (time.perf_counter() - t0))
        tr = np.ascontiguousarray(tr)
        t0 = time.perf_counter()
        assert lib.vdf_dev_memcpy(ctx.handle, d_trace.data_ptr(), tr.ctypes.data, tr.nbytes) == 0
        ctx.sync()
        cp_ms.append(1e3 * (time.perf_counter() - t0))
    out("(2) per step from checkpoints: k_tape_walk %.3f ms + k_round_tape %.3f ms = %.3f ms on the device, %d bytes uploaded" % (
        w_ms, r_ms, w_ms + r_ms, 2 * per * 64))
    out("    per step from a host trace: vdf_minroot_eval %.1f ms + vdf_dev_memcpy of %d bytes %.3f ms (+ k_round_tape %.3f ms)" % (
        statistics.median(ev_ms), tr.nbytes, statistics.median(cp_ms), r_ms))
    # ---- (3) the prove_step_custom rate, both ways
    host_traces = []
    for g in range(a.steps):                                    # the traces of way B, by the host evaluator of the same tape
        e, buf = xy[g * per + 1:g * per + per + 1].reshape(-1, 4).copy(), np.zeros((2 * (t + 1), 4), dtype="<u8")
        walk_tape_eval(FIELD_FQ, walk_tape, i0, e, per, every, buf, walk_stride=every, top=every, group=per, group_stride=t + 1, j_base=g * t,
                       heads=True)
        host_traces.append(buf)
    c = F(t, "repeat")
    pp = public_params_custom(ctx, c)

    def run(way):
        proof, t0 = None, None
        for g in range(a.steps):
            if g == a.warmup:
                ctx.sync()
                t0 = time.perf_counter()
            if way == "walk":
                walk_step(g)
            else:
                assert lib.vdf_dev_memcpy(ctx.handle, d_trace.data_ptr(), host_traces[g].ctypes.data, host_traces[g].nbytes) == 0
            c.advice = d_trace
            proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
        ctx.sync()
        rate = (a.steps - a.warmup) / (time.perf_counter() - t0)
        assert proof.verify(pp, a.steps, z0, zi) is True, way
        proof.free()
        return rate
    rates = {"walk": [], "upload": []}
    for _ in range(a.runs):
        for way in rates:
            rates[way].append(run(way))
    for way, label in (("walk", "advice by a walk from checkpoints"), ("upload", "advice uploaded from a host trace")):
        r = rates[way]
        out("(3) %-36s %s steps/s: median %.2f, min %.2f, max %.2f" % (label + ":", " ".join("%.2f" % x for x in r), statistics.median(r), min(r), max(r)))
    out("    walk / upload: %.3fx in steps per second over %d steps after %d (the upload path's evaluation, (2), is not in its loop)" % (
        statistics.median(rates["walk"]) / statistics.median(rates["upload"]), a.steps - a.warmup, a.warmup))
    pp.free()
    ctx.close()


if __name__ == "__main__":
    main()
