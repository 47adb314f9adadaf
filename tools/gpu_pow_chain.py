#!/usr/bin/env python3
"""Measurement of powers by an addition chain in forward walk tapes (VDF_TAPE_POWC, k_tape_forward_walk_chain) on one MI355X,
profiler off (output: profiles/r19_pow_chain.txt).  tools/gpu_custom_forward.py's setup, so that the figures line up with
profiles/r15_custom_forward.txt: one process, no child process, `--chains` chains (default 2^16) of `--rounds` rounds (default 64)
of the MinRoot forward round over Fq.  Run it under a time limit of its own:

  timeout -k 10 300 python3 tools/gpu_pow_chain.py

  (1) four arrangements on the same chains, a warm-up and `--repeats` (default 5) ALTERNATING repeats, per-launch HIP events:
        (a) the tape with VDF_TAPE_POW (binary square-and-multiply, 377 products) through the unchanged k_tape_forward_walk: the
            yardstick, the parent's path
        (b) the tape with VDF_TAPE_POWC over vdf_minroot_pow_chain (the reference's chain, 283 products) through
            k_tape_forward_walk_chain
        (c) POWC over vdf_nova_pow_chain_window(e, 4) (316 products)
        (d) vdf_minroot_forward_walk, the hand-written k_forward_walk
      median, minimum and maximum of each, us per round and lane, (b)/(a), (c)/(a), (b)/(d), and whether (b)'s maximum lies below
      (a)'s minimum.  The landings of all four are compared byte for byte.
  (2) the same tape on ONE host core through vdf_nova_forward_tape_eval, with POW and with POWC."""
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-chains", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_pow_chain.txt"))
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
    from vdf_amd import minroot
    from vdf_amd.minroot import FIELD_FQ
    from vdf_amd.nova import forward_tape_eval, pow_chain_exponent, pow_chain_window, record_forward_body
    from forward_tape_spec import minroot_forward_body, pow_products, root_exponent
    from pow_chain_spec import minroot_chain_body
    from rounds_spec import MOD
    from util import dev, host, mont_states
    out("powers by an addition chain in forward walk tapes on %s, %d chains x %d rounds; GPU_MAX_HW_QUEUES = %s" % (
        torch.cuda.get_device_name(0), n, rounds, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    m, i0, e = MOD[FIELD_FQ], 7, root_exponent(FIELD_FQ)
    chains = {"b": minroot.pow_chain(FIELD_FQ), "c": pow_chain_window(e, 4)}
    tapes = {"a": record_forward_body(minroot_forward_body(FIELD_FQ))}
    out("(a) POW: %d products; %d slots + 2 x %d columns = %d KiB of LDS per wavefront" % (
        pow_products(e), tapes["a"].c.n_slots, tapes["a"].c.n_adv, 2 * (tapes["a"].c.n_slots + 2 * tapes["a"].c.n_adv)))
    for k, what in (("b", "vdf_minroot_pow_chain"), ("c", "vdf_nova_pow_chain_window(e, 4)")):
        tapes[k] = record_forward_body(minroot_chain_body(FIELD_FQ, chains[k]))
        E, n_tmp, products = pow_chain_exponent(chains[k])
        assert E == e
        out("(%s) POWC over %s: %d steps, %d products; %d slots + 2 x %d columns + %d temporaries = %d KiB of LDS per wavefront" % (
            k, what, len(chains[k]), products, tapes[k].c.n_slots, tapes[k].c.n_adv, n_tmp,
            2 * (tapes[k].c.n_slots + 2 * tapes[k].c.n_adv + n_tmp)))
    rng = np.random.default_rng(15)
    xy = rng.integers(1, 2**62, size=(n, 2))
    states = mont_states([[int(xy[w, 0]) ** 4 % m, int(xy[w, 1]) ** 3 % m, i0 + 1000 * w] for w in range(n)], m)
    start = np.ascontiguousarray(states[:, :8])
    d_states0, d_entries0 = dev(states), dev(start)
    # ---- (1) the four arrangements on the same chains, alternating
    ctx.set_kernel_timing(True)
    order, land = [], {}
    for _ in range(a.repeats + 1):                                  # the first pass is the warm-up
        for k in ("a", "b", "c"):
            land[k] = d_entries0.clone()
            ctx.round_tape_forward_walk(FIELD_FQ, tapes[k], None, land[k], n, rounds, j_base=i0, j_walk_step=1000)
            order.append(k)
        land["d"] = d_states0.clone()
        ctx.minroot_forward_walk(FIELD_FQ, land["d"], n, rounds)
        order.append("d")
    ctx.sync()
    ev = ctx.kernel_events()
    ctx.set_kernel_timing(False)
    assert len(ev) == len(order)
    want = np.ascontiguousarray(host(land["d"]).reshape(n, 12)[:, :8]).tobytes()
    same = all(host(land[k]).reshape(n, 8).tobytes() == want for k in "abc")
    out("    landings of the four byte for byte equal: %s" % same)
    assert same
    kernel = {"a": "k_tape_forward_walk", "b": "k_tape_forward_walk_chain"[:23], "c": "k_tape_forward_walk_chain"[:23], "d": "k_forward_walk"}
    ms = {k: [] for k in "abcd"}
    for k, e_ in list(zip(order, ev))[4:]:
        assert e_[0] == kernel[k], (k, e_[0])
        ms[k].append(e_[3] - e_[2])
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in "abcd":
        out("(1) (%s) %-25s %d launches: median %.3f ms, min %.3f, max %.3f -> %.2f us per round and lane, %.1f M rounds/s" % (
            k, "k_tape_forward_walk_chain" if k in "bc" else kernel[k], len(ms[k]), med[k], min(ms[k]), max(ms[k]), 1e3 * med[k] / rounds,
            n * rounds / med[k] / 1e3))
    out("    (b)/(a) = %.3f (product counts alone: 283/377 = 0.751), (c)/(a) = %.3f (316/377 = 0.838), (b)/(d) = %.3f" % (
        med["b"] / med["a"], med["c"] / med["a"], med["b"] / med["d"]))
    out("    (b)'s maximum %s (a)'s minimum: %.3f ms against %.3f ms" % (
        "lies below" if max(ms["b"]) < min(ms["a"]) else "does NOT lie below", max(ms["b"]), min(ms["a"])))
    # ---- (2) the same tape on one host core
    hn = min(a.host_chains, n)
    for k in ("a", "b"):
        secs = []
        for _ in range(3):
            x = start[:hn].reshape(-1, 4).copy()
            t0 = time.perf_counter()
            forward_tape_eval(FIELD_FQ, tapes[k], None, x, hn, rounds, j_base=i0, j_walk_step=1000)
            secs.append(time.perf_counter() - t0)
        assert x.tobytes() == want[:64 * hn]
        hs = statistics.median(secs)
        out("(2) (%s) vdf_nova_forward_tape_eval, one host core, %d chains x %d rounds: median %.1f ms -> %.2f us per round; one chain: the "
            "device lane takes %.1fx the host core's time per round" % (k, hn, rounds, 1e3 * hs, 1e6 * hs / (hn * rounds),
                                                                        (1e3 * med[k] / rounds) / (1e6 * hs / (hn * rounds))))
    ctx.close()


if __name__ == "__main__":
    main()
