#!/usr/bin/env python3
"""Measurements of forward walk tapes (vdf_round_tape_forward_walk, k_tape_forward_walk) on one MI355X, profiler off (output:
profiles/r15_custom_forward.txt).  One process, no child process; run it under a time limit of its own:

  timeout -k 10 300 python3 tools/gpu_custom_forward.py

`--chains` chains (default 2^16) of `--rounds` rounds (default 64), so that the whole tool takes seconds.

  (1) k_tape_forward_walk running the MinRoot forward round as a tape (one POW: binary exponentiation by 5^-1 mod (m - 1)) beside
      k_forward_walk, the hand-written kernel (the reference's addition chain), on the same chains: per-launch HIP events,
      medians, the time per round of a lane (a lane's rounds are sequential, the lanes run side by side) and rounds per second
      over all lanes.  The landings of the two are compared byte for byte.  README's yardstick for k_forward_walk is 114 us per
      round of one chain.  How far the interpreter lands from the hand-written walk is reported, not bounded.
  (2) the same tape on ONE host core: vdf_nova_forward_tape_eval over `--host-chains` of the chains, in rounds per second,
      against the device's."""
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
    ap.add_argument("--chains", type=int, default=1 << 16)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--host-chains", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_custom_forward.txt"))
    a = ap.parse_args()
    n, rounds = a.chains, a.rounds
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "w")

    def out(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    import numpy as np
    import torch
    import vdf_amd
    from vdf_amd.minroot import FIELD_FQ
    from vdf_amd.nova import forward_tape_eval, record_forward_body
    from forward_tape_spec import minroot_forward_body, pow_products, root_exponent
    from rounds_spec import MOD
    from util import dev, host, mont_states
    out("forward walk tapes on %s, %d chains x %d rounds; GPU_MAX_HW_QUEUES = %s" % (
        torch.cuda.get_device_name(0), n, rounds, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    m, i0 = MOD[FIELD_FQ], 7
    tape = record_forward_body(minroot_forward_body(FIELD_FQ))
    out("forward tape: %d ops, one POW of %d products (bitlen - 1 squarings + popcount - 1 products), %d slots + 2 x %d columns = %d KiB "
        "of LDS per wavefront" % (len(tape.op_list()), pow_products(root_exponent(FIELD_FQ)), tape.c.n_slots, tape.c.n_adv,
                                  2 * (tape.c.n_slots + 2 * tape.c.n_adv)))
    rng = np.random.default_rng(15)
    xy = rng.integers(1, 2**62, size=(n, 2))
    states = mont_states([[int(xy[w, 0]) ** 4 % m, int(xy[w, 1]) ** 3 % m, i0 + 1000 * w] for w in range(n)], m)
    start = np.ascontiguousarray(states[:, :8])
    d_states0, d_entries0 = dev(states), dev(start)
    # ---- (1) the two kernels on the same chains
    ctx.set_kernel_timing(True)
    for _ in range(a.launches + 1):
        d_entries, d_states = d_entries0.clone(), d_states0.clone()
        ctx.round_tape_forward_walk(FIELD_FQ, tape, None, d_entries, n, rounds, j_base=i0, j_walk_step=1000)
        ctx.minroot_forward_walk(FIELD_FQ, d_states, n, rounds)
    ctx.sync()
    ev = ctx.kernel_events()
    ctx.set_kernel_timing(False)
    same = host(d_entries).reshape(n, 8).tobytes() == np.ascontiguousarray(host(d_states).reshape(n, 12)[:, :8]).tobytes()
    out("    landings of the two kernels byte for byte equal: %s" % same)
    assert same
    med = {}
    for name in ("k_tape_forward_walk", "k_forward_walk"):
        d = [e[3] - e[2] for e in ev if e[0] == name][1:]
        med[name] = statistics.median(d)
        out("(1) %-20s %d launches: median %.3f ms, min %.3f, max %.3f -> %.2f us per round and lane, %.1f M rounds/s" % (
            name, len(d), med[name], min(d), max(d), 1e3 * med[name] / rounds, n * rounds / med[name] / 1e3))
    out("    interpreter / hand-written walk: %.2fx (yardstick: 114 us per round for one chain, 659 M rounds/s at 524,288 chains)" % (
        med["k_tape_forward_walk"] / med["k_forward_walk"]))
    # ---- (2) the same tape on one host core
    hn = min(a.host_chains, n)
    secs = []
    for _ in range(3):
        e = start[:hn].reshape(-1, 4).copy()
        t0 = time.perf_counter()
        forward_tape_eval(FIELD_FQ, tape, None, e, hn, rounds, j_base=i0, j_walk_step=1000)
        secs.append(time.perf_counter() - t0)
    assert e.tobytes() == host(d_entries).reshape(n, 8)[:hn].tobytes()
    hs = statistics.median(secs)
    host_rate, dev_rate = hn * rounds / hs, n * rounds / (med["k_tape_forward_walk"] / 1e3)
    out("(2) vdf_nova_forward_tape_eval, one host core, %d chains x %d rounds: median %.1f ms -> %.2f us per round, %.3f M rounds/s" % (
        hn, rounds, 1e3 * hs, 1e6 * hs / (hn * rounds), host_rate / 1e6))
    out("    one chain: the device lane takes %.1fx the host core's time per round; %d chains: the device makes %.0fx the host core's rounds per second" % (
        (1e3 * med["k_tape_forward_walk"] / rounds) / (1e6 * hs / (hn * rounds)), n, dev_rate / host_rate))
    ctx.close()


if __name__ == "__main__":
    main()
