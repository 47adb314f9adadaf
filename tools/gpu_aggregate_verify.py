"""Verifying an aggregate of K proofs from its bytes, the host way against the device way, at t = 2^16 on the reference's circuit:
K in {1, 2, 16, 128, 1024}, a few distinct proofs named cyclically (a proof named twice is folded twice), in one process, the two
ways taking turns repeat by repeat.
  host way    = vdf_nova_aggregate_deserialize + vdf_nova_verify_aggregate       (the reference: host point arithmetic per entry)
  device way  = vdf_nova_verify_aggregate_wire                                   (decoding, per-entry folds and sums on the GPU)
Per K: both ways' wall time as median [min .. max]; the device call's parts as the library clocks them on the host
(vdf_nova_aggregate_verify_times: decoding, the exact checks = three Poseidon hashes per entry, the secondary folds, both
accumulators, both arguments) beside the kernel events (KTimer) of k_points_decompress and k_points_axpy and of every other
launch of one more call; and k_points_axpy alone at n = 2 K for both scalar lengths.
THE RULE: "faster at K" is claimed only where the device way's slowest repeat is below the host way's fastest; the K where it is
not are listed as such.  Every K runs under a time limit of its own (--step-timeout, a watchdog that ends the process).
--ro-device: the other comparison, same K set and method -- the device way with its per-entry Poseidon hashes on the host
(vdf_nova_pp_set_verify_ro_device at 0) against the same call with the switch at 1 (three vdf_ro_hash_batch launches), taking
turns repeat by repeat; per K both wall times, both ways' parts, k_ro_hash by events (one more call, and alone at n = K for the
three message lengths of an aggregate), and the rule with "switch at 1" in the place of the device way and "switch at 0" in
the place of the host way.  The smallest K of an unbroken run of "yes" up to the largest K is the min_count to recommend.
--ro-block: the same comparison under the neptune-shaped parameter set (family 1: width 25, 8 + 57 rounds) -- the device way
with vdf_nova_pp_set_verify_ro_block_device at 0 (the host hashes) against the same call with that switch at 1 (three
vdf_ro_hash_batch_block launches); k_ro_hash_block by events, and alone at n = K for the three message lengths.
usage: python tools/gpu_aggregate_verify.py [--lg 16] [--ks 1,2,16,128,1024] [--proofs 4] [--repeats 5] [--step-timeout 240] [--out FILE]
                                            [--ro-device | --ro-block]"""
import argparse
import os
import signal
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
from gpu_verify_multi_time import kernel_figures  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=16)
    ap.add_argument("--ks", default="1,2,16,128,1024")
    ap.add_argument("--proofs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ro-device", action="store_true")
    ap.add_argument("--ro-block", action="store_true")
    a = ap.parse_args()
    if a.ro_device and a.ro_block:
        ap.error("--ro-device and --ro-block are two runs")
    import numpy as np
    import torch
    import vdf_amd
    from oracle import pasta as o
    from vdf_amd import _lib
    from vdf_amd.minroot import EvalMode, PallasVDF, State, FIELD_FQ
    from vdf_amd.nova import (InverseMinRootCircuit, NovaVDFProof, aggregate_verify_times, compress_aggregate, deserialize_aggregate, public_params,
                              RO_NEPTUNE_SHAPED, ro_block_constants, ro_constants, ro_preset, verify_aggregate_wire)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def overdue(signum, frame):
        say("a step ran past its time limit: the run ends here")
        save()
        os._exit(3)
    signal.signal(signal.SIGALRM, overdue)

    t = 1 << a.lg
    ks = [int(x) for x in a.ks.split(",") if x]
    signal.alarm(a.step_timeout)
    ctx = vdf_amd.Context(0)
    ro = ro_preset(RO_NEPTUNE_SHAPED) if a.ro_block else None
    pp = public_params(ctx, t, ro=ro)
    # which switch the run turns, the kernel it watches and that kernel alone at n messages
    set_switch = pp.set_verify_ro_block_device if a.ro_block else pp.set_verify_ro_device
    kernel = "k_ro_hash_block" if a.ro_block else "k_ro_hash"
    items = []
    for q in range(a.proofs):                              # distinct chains of 1, 2, 1, 2, ... steps
        n = 1 + q % 2
        init = State.from_ints(FIELD_FQ, o.rand_fe(9100 + q, 0, o.Q), 0, 1)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential), t, n, init)
        items.append((NovaVDFProof.prove_recursively(pp, circuits, t, z0), n, z0, [init.x, init.y, init.i]))
    signal.alarm(0)
    say(f"t = 2^{a.lg}, {a.proofs} distinct proofs named cyclically, {a.repeats} alternating repeats in one process; ms as median [min .. max]")
    fmt = lambda v: "%9.2f [%9.2f .. %9.2f]" % (statistics.median(v), min(v), max(v))
    faster, not_faster = [], []
    PARTS = ("exact checks and hashes", "secondary folds", "both accumulators", "both arguments", "decoding")

    def ro_device_at(K, data, stmt):
        ways = (("switch at 0", 0), ("switch at 1", 1))
        for _, sw in ways:                                 # warm both ways (the second makes the constants' device copies)
            set_switch(sw)
            if verify_aggregate_wire(pp, data, *stmt) != (True, -1, 0):
                sys.exit(f"K = {K}: the aggregate does not verify")
        tm = {name: [] for name, _ in ways}
        parts = {name: [] for name, _ in ways}
        for _ in range(a.repeats):
            for name, sw in ways:
                set_switch(sw)
                ctx.sync(); t0 = time.perf_counter()
                wired = verify_aggregate_wire(pp, data, *stmt); ctx.sync()
                tm[name].append(1e3 * (time.perf_counter() - t0))
                parts[name].append(aggregate_verify_times())
                if wired != (True, -1, 0):
                    sys.exit(f"K = {K}: the aggregate does not verify")
        say(f"K = {K:4d}   {len(data)} bytes")
        for name, v in tm.items():
            say(f"   device way, {name} ms {fmt(v)}   per entry {statistics.median(v) / K:8.3f}")
        ok = max(tm["switch at 1"]) < min(tm["switch at 0"])
        (faster if ok else not_faster).append(K)
        say(f"   switch at 1 faster by the rule (its slowest repeat below the fastest with the switch at 0): {'yes' if ok else 'NO'}")
        for name, _ in ways:
            for j, part in enumerate(PARTS):
                say(f"   {name}, {part:24s} ms {fmt([p[j] for p in parts[name]])}")
        set_switch(1)                                      # one more call with the library's events around its launches
        before = pp.verify_ro_stats()
        ctx.set_kernel_timing(True)
        ctx.kernel_events()
        verify_aggregate_wire(pp, data, *stmt)
        ctx.sync()
        ev = ctx.kernel_events()
        ctx.set_kernel_timing(False)
        after = pp.verify_ro_stats()
        set_switch(0)
        ms = [e1 - e0 for kn, _, e0, e1 in ev if kn == kernel]
        say(f"   events: {kernel} {len(ms):3d} launches, {sum(ms):9.3f} ms ({', '.join('%.3f' % v for v in ms)});"
            f" stats: {after[0] - before[0]} hashes in {after[1] - before[1]} launches")
        rng = np.random.default_rng(K)                     # the kernel alone at n = K, device arrays, the aggregate's three lengths
        if a.ro_block:
            rc, mds = (torch.from_numpy(c.view(np.int64)).cuda() for c in ro_block_constants(FIELD_FQ, ro))
            alone = lambda dxs, ln, bits, out: ctx.ro_hash_batch_block(FIELD_FQ, 1, ro.width, ro.full_rounds, ro.partial_rounds, rc, mds, dxs, ln, K,
                                                                       bits, out)
        else:
            rc = torch.from_numpy(ro_constants(FIELD_FQ).view(np.int64)).cuda()
            alone = lambda dxs, ln, bits, out: ctx.ro_hash_batch(FIELD_FQ, 1, rc, dxs, ln, K, bits, out)
        out = torch.zeros((K, 4), dtype=torch.int64, device="cuda")
        for ln, bits in ((17, 250), (13, 250), (16, 128)):
            xs = rng.integers(0, 2**62, size=(K * ln, 4), dtype=np.int64)
            xs[:, 3] &= 0x3FFFFFFFFFFFFFFF
            dxs = torch.from_numpy(xs).cuda()
            ctx.set_kernel_timing(True)
            ctx.kernel_events()
            for _ in range(a.repeats + 1):
                alone(dxs, ln, bits, out)
            ctx.sync()
            us = [1e3 * (e1 - e0) for kn, _, e0, e1 in ctx.kernel_events() if kn == kernel][1:]
            ctx.set_kernel_timing(False)
            say(f"   {kernel} alone, n = {K:4d}, len = {ln:2d}, bits = {bits:3d}: us {statistics.median(us):9.1f} [{min(us):9.1f} .. {max(us):9.1f}]")

    for K in ks:
        signal.alarm(a.step_timeout)
        its = [items[k % a.proofs] for k in range(K)]
        stmt = ([it[1] for it in its], [it[2] for it in its], [it[3] for it in its])
        agg = compress_aggregate(pp, [it[0] for it in its])
        data = agg.serialize()
        agg.free()
        if deserialize_aggregate(pp, data).verify(pp, *stmt) != (True, -1) or verify_aggregate_wire(pp, data, *stmt) != (True, -1, 0):   # warm both ways
            sys.exit(f"K = {K}: the aggregate does not verify")
        if a.ro_device or a.ro_block:
            ro_device_at(K, data, stmt)
            signal.alarm(0)
            save()
            continue
        tm = {"host way": [], "device way": []}
        parts = []
        for _ in range(a.repeats):
            ctx.sync(); t0 = time.perf_counter()
            back = deserialize_aggregate(pp, data); verdict = back.verify(pp, *stmt); ctx.sync()
            tm["host way"].append(1e3 * (time.perf_counter() - t0))
            back.free()
            t0 = time.perf_counter()
            wired = verify_aggregate_wire(pp, data, *stmt); ctx.sync()
            tm["device way"].append(1e3 * (time.perf_counter() - t0))
            parts.append(aggregate_verify_times())
            if verdict != (True, -1) or wired != (True, -1, 0):
                sys.exit(f"K = {K}: the aggregate does not verify")
        say(f"K = {K:4d}   {len(data)} bytes")
        for k, v in tm.items():
            say(f"   {k:11s} ms {fmt(v)}   per entry {statistics.median(v) / K:8.3f}")
        ok = max(tm["device way"]) < min(tm["host way"])
        (faster if ok else not_faster).append(K)
        say(f"   device way faster by the rule (its slowest repeat below the host way's fastest): {'yes' if ok else 'NO'}")
        for j, name in enumerate(("exact checks and hashes (host)", "secondary folds", "both accumulators", "both arguments", "decoding")):
            say(f"   device way, {name:31s} ms {fmt([p[j] for p in parts])}")
        # one more call with the library's events around its launches
        ctx.set_kernel_timing(True)
        ctx.kernel_events()
        verify_aggregate_wire(pp, data, *stmt)
        ctx.sync()
        ev = ctx.kernel_events()
        ctx.set_kernel_timing(False)
        for name in ("k_points_decompress", "k_points_axpy"):
            ms = [e1 - e0 for kn, _, e0, e1 in ev if kn == name]
            say(f"   events: {name:20s} {len(ms):3d} launches, {sum(ms):9.3f} ms")
        rest = [e1 - e0 for kn, _, e0, e1 in ev if kn not in ("k_points_decompress", "k_points_axpy")]
        say(f"   events: every other kernel    {len(rest):3d} launches, {sum(rest):9.3f} ms   (the accumulators' sums and the arguments)")
        # the per-entry kernel alone at n = 2 K, device arrays: the aggregate's own points are not needed for its time
        n = 2 * K
        bases = ctx.bases_generate(vdf_amd.CURVE_VESTA, 5, 2 * n)
        pts = torch.from_numpy(bases.download().view(np.int64)).cuda()
        bases.free()
        rng = np.random.default_rng(K)
        sc = torch.from_numpy(rng.integers(0, 2**63, size=(n, 4), dtype=np.int64)).cuda()
        out = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        for bits in (128, 255):
            ctx.set_kernel_timing(True)
            ctx.kernel_events()
            for _ in range(a.repeats + 1):
                ctx.points_axpy(vdf_amd.CURVE_VESTA, pts[:n], pts[n:], sc, bits, n, out)
            ctx.sync()
            us = [1e3 * (e1 - e0) for kn, _, e0, e1 in ctx.kernel_events() if kn == "k_points_axpy"][1:]
            ctx.set_kernel_timing(False)
            say(f"   k_points_axpy alone, n = {n:4d}, bits = {bits:3d}: us {statistics.median(us):9.1f} [{min(us):9.1f} .. {max(us):9.1f}]")
        signal.alarm(0)
        save()
    if a.ro_device or a.ro_block:
        say(f"switch at 1 faster by the rule at K in {faster}; not faster at K in {not_faster}")
    else:
        say(f"device way faster by the rule at K in {faster}; not faster at K in {not_faster}")
    for sym, vgpr, agpr, lds, scratch in kernel_figures(_lib.lib._name, kernel if a.ro_device or a.ro_block else "k_points_axpy"):
        say(f"{sym}: {vgpr} VGPRs, {agpr} AGPRs, {lds} B LDS, {scratch} B scratch")
    save()


if __name__ == "__main__":
    main()
