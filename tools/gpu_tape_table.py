#!/usr/bin/env python3
"""ONE measurement of VDF_TAPE_TAB on one MI355X, profiler off (output: profiles/r23_tape_table.txt): what reading the round
constant from a table costs beside VDF_TAPE_J.  The MinRoot forward, walk and round tapes as they are, against the same tapes with
their counter read from a table whose entry r is the field element r -- the same values, so the walks' landings are compared byte
for byte -- through the kernels a tabbed tape launches (k_tape_forward_walk_tab, k_tape_walk_tab, k_round_tape_tab).  One process,
no child process, a warm-up and `--repeats` (default 5) ALTERNATING repeats, per-launch HIP events.  Run it under a time limit:

  timeout -k 10 300 python3 tools/gpu_tape_table.py

  forward  `--chains` (2^16) chains x `--rounds` (64) rounds of x' = (x + y)^(1/5), y' = x + j  (POW)     table: 64 rows
  walk     the same chains back down: x = y' - (i0 + j), y = x'^5 - x                                    table: 64 rows
  round    t = 2^16 repetitions of the forward MinRoot round with y' = x + i + j made a variable (the round tape as it is reads
           no counter: its y' is a linear combination, and a value no variable depends on gets no op)     table: 4096 rows (the cap)
No threshold: a capability, measured once."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1 << 16)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--t", type=int, default=1 << 16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_tape_table.txt"))
    a = ap.parse_args()
    n, rounds, t = a.chains, a.rounds, a.t
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
    from vdf_amd.nova import RoundBody, WalkBody, record_forward_body, record_round_body, record_walk_body
    from forward_tape_spec import minroot_forward_body, root_exponent
    from rounds_spec import MOD, mont_rows
    from tab_spec import table_array
    from util import dev, host
    from walks_spec import minroot_body
    field, m, i0 = FIELD_FQ, MOD[FIELD_FQ], 7
    out("VDF_TAPE_TAB beside VDF_TAPE_J on %s: %d chains x %d rounds (walks), t = %d (round kernel); GPU_MAX_HW_QUEUES = %s" % (
        torch.cuda.get_device_name(0), n, rounds, t, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    T64 = table_array(list(range(rounds)), rounds, 1, m)
    T4096 = table_array(list(range(4096)), 4096, 1, m)
    e = root_exponent(field)

    def walk_tab(cs, j, inv, nxt):
        cx = cs.sub(nxt[1], cs.add(inv[0], cs.tab(T64, 0)))
        x2 = cs.mul(nxt[0], nxt[0])
        return [cx, cs.sub(cs.mul(cs.mul(x2, x2), nxt[0]), cx)]

    def round_of(counter):
        def b(cs, j, inv, carry, cur, nxt):
            x, y = carry
            xn = cs.alloc_from(nxt[0])
            t1 = cs.mul(xn, xn)
            t2 = cs.mul(t1, t1)
            cs.enforce(t2, xn, cs.add(x, y))
            return [xn, cs.alloc_from(cs.add(cs.add(x, inv[0]), counter(cs, j)))]
        return RoundBody(1, 2, 2, b)
    tapes = {
        "forward": (record_forward_body(minroot_forward_body(field)),
                    record_forward_body(WalkBody(0, 2, lambda cs, j, inv, cur: [cs.pow(cs.add(cur[0], cur[1]), e), cs.add(cur[0], cs.tab(T64, 0))]))),
        "walk": (record_walk_body(minroot_body(field)), record_walk_body(WalkBody(1, 2, walk_tab))),
        "round": (record_round_body(round_of(lambda cs, j: j)), record_round_body(round_of(lambda cs, j: cs.tab(T4096, 0)))),
    }
    kernel = {"forward": ("k_tape_forward_walk", "k_tape_forward_walk_tab"), "walk": ("k_tape_walk", "k_tape_walk_tab"),
              "round": ("k_round_tape", "k_round_tape_tab")}
    for k, (plain, tab) in tapes.items():
        out("%-8s as it is: %d ops, %d slots; with the table: %d ops, %d slots, %d x %d elements" % (
            k, plain.c.n_ops, plain.c.n_slots, tab.c.n_ops, tab.c.n_slots, tab.c.tab_rows, tab.c.tab_cols))
    rng = np.random.default_rng(23)
    xy = rng.integers(1, 2**62, size=(n, 2))
    start = mont_rows([int(v) ** 3 % m for v in xy.reshape(-1)], m)
    d_start = dev(start)
    inv = mont_rows([i0], m)
    adv = rng.integers(0, 2**62, size=((t + 1) * 2, 4)).astype("<u8")       # any canonical elements: the round kernel checks nothing
    d_adv = dev(adv)
    n_vars = tapes["round"][0].c.n_vars
    d_out = [torch.zeros((t * n_vars, 4), dtype=torch.int64, device="cuda") for _ in range(2)]
    ctx.set_kernel_timing(True)
    ctx.kernel_events()
    order, top = [], {}
    for _ in range(a.repeats + 1):                                  # the first pass is the warm-up
        for v in (0, 1):
            top[v] = d_start.clone()
            # the plain forward tape adds j itself, the plain walk tape inv + j: both chains count from 0 under the forward tape
            ctx.round_tape_forward_walk(field, tapes["forward"][v], None, top[v], n, rounds)
            order.append(("forward", v))
        for v in (0, 1):
            top[2 + v] = top[v].clone()
            ctx.round_tape_walk(field, tapes["walk"][v], mont_rows([0], m), top[2 + v], n, rounds, top=rounds)
            order.append(("walk", v))
        for v in (0, 1):
            ctx.round_tape_run(field, tapes["round"][v], t, inv, d_adv, d_out[v])
            order.append(("round", v))
    ctx.sync()
    ev = ctx.kernel_events()
    ctx.set_kernel_timing(False)
    assert len(ev) == len(order), (len(ev), len(order))
    same = host(top[0]).tobytes() == host(top[1]).tobytes() and host(top[2]).tobytes() == host(top[3]).tobytes() == start.tobytes()
    first = 4096 * n_vars
    same_round = host(d_out[0])[:first].tobytes() == host(d_out[1])[:first].tobytes()
    out("landings of the forward walks equal, and of the walks back down equal to the start: %s; the first 4096 repetitions of the "
        "round kernel equal: %s" % (same, same_round))
    assert same and same_round
    ms = {}
    for (k, v), e_ in list(zip(order, ev))[6:]:
        assert e_[0] == kernel[k][v], (k, v, e_[0])
        ms.setdefault((k, v), []).append(e_[3] - e_[2])
    for k in ("forward", "walk", "round"):
        med = [statistics.median(ms[(k, v)]) for v in (0, 1)]
        for v in (0, 1):
            x = ms[(k, v)]
            out("%-8s %-24s %d launches: median %.3f ms, min %.3f, max %.3f" % (k, kernel[k][v], len(x), med[v], min(x), max(x)))
        out("%-8s with the table / as it is = %.3f" % (k, med[1] / med[0]))
    ctx.close()


if __name__ == "__main__":
    main()
