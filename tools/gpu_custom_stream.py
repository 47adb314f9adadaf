#!/usr/bin/env python3
"""Measurement of vdf_nova_eval_and_prove_custom on one MI355X, profiler off (output: profiles/r25_custom_stream.txt).  ONE process;
the arrangements alternate inside every repeat.  Every figure is reported, none is gated.

  Workload: the MinRoot forward round as a tape with the library's addition chain, t = 2^16, 16 steps, one lane, proved while library
  threads evaluate it, by three hand-overs:
    traces       every = 0: whole traces are handed over and uploaded
    ascending    checkpoints every 64 rounds, rebuilt on the device by the forward tape itself
    descending   checkpoints every 4,096 rounds, rebuilt by the inverse walk tape
  and beside them the built-in vdf_nova_eval_and_prove (the forward MinRoot circuit, the library's own evaluator) over the same chain.
  Reported per arrangement: eval_ms, after_eval_ms and max_backlog as min / median / max.  What matters is after_eval_ms: the distance
  from the chain's output to its proof."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--log2t", type=int, default=16)
    ap.add_argument("--ascending-every", type=int, default=64)
    ap.add_argument("--descending-every", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_custom_stream.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    log = open(a.out, "w")

    def out(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    import vdf_amd
    from vdf_amd.minroot import FIELD_FQ, EvalMode, PallasVDF, State, pow_chain
    from vdf_amd.nova import (CIRCUIT_MINROOT_FORWARD, NovaVDFProof, WalkBody, public_params, public_params_custom, record_forward_body,
                              record_walk_body)
    from custom_chain_spec import FC
    from rounds_spec import MOD, mont_rows
    from walks_spec import minroot_body
    t, steps = 1 << a.log2t, a.steps
    out("a custom chain proved while it is evaluated: t = 2^%d, %d steps, one lane, %d alternating repeats; GPU_MAX_HW_QUEUES = %s" % (
        a.log2t, steps, a.runs, os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")))
    ctx = vdf_amd.Context(0)
    m, x0, i0 = MOD[FIELD_FQ], 0x51DE, 7
    chain5 = pow_chain(FIELD_FQ)
    # x' = (x + y)^(1/5) by the library's chain, y' = x + i0 + j: the round walks_spec.minroot_body inverts
    fwd = record_forward_body(WalkBody(1, 2, lambda cs, j, inv, cur: [cs.pow_chain(cs.add(cur[0], cur[1]), chain5), cs.add(cur[0], cs.add(inv[0], j))]), FIELD_FQ)
    walk = record_walk_body(minroot_body(FIELD_FQ), FIELD_FQ)
    inv, initial = mont_rows([i0], m), mont_rows([x0, 0], m)
    z0 = [mont_rows([v], m).tobytes() for v in (x0, 0, i0)]
    c = FC(t)
    pp = public_params_custom(ctx, c)
    ppf = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)
    first = State.from_ints(FIELD_FQ, x0, 0, i0)
    vdf = PallasVDF.new_with_mode(EvalMode.LTRAddChainSequential)

    def custom(every, walk_tape, n=steps):
        proof, final, st = NovaVDFProof.eval_and_prove_custom(pp, c, fwd, inv, t, initial, n, z0, every=every, walk_tape=walk_tape,
                                                              walk_inv=inv if walk_tape is not None else None)
        return proof, final.tobytes(), st

    def builtin(n=steps):
        proof, last, st = NovaVDFProof.eval_and_prove(ppf, vdf, first, n)
        return proof, last.x + last.y, st
    runs = (("traces", lambda n=steps: custom(0, None, n)),
            ("ascending, every %d" % a.ascending_every, lambda n=steps: custom(a.ascending_every, None, n)),
            ("descending, every %d" % a.descending_every, lambda n=steps: custom(a.descending_every, walk, n)),
            ("built-in eval_and_prove", builtin))
    # once untimed over two steps: queues, buffers, the table of generators; the arrangements agree on where the chain ends
    ends = []
    for name, run in runs:
        proof, end, _ = run(2)
        ends.append(end)
        proof.free()
    assert len(set(ends)) == 1, "the arrangements end on different states"
    want, r = None, {name: [] for name, _ in runs}
    for _ in range(a.runs):
        for name, run in runs:
            proof, end, st = run()
            if name != runs[-1][0]:                      # the three hand-overs give ONE proof
                got = proof.serialize()
                want = got if want is None else want
                assert got == want, "the proof of '%s' differs" % name
            proof.free()
            r[name].append(st)
    for name, _ in runs:
        def mmm(key, fmt):
            v = [s[key] for s in r[name]]
            return "%s / %s / %s" % (fmt % min(v), fmt % statistics.median(v), fmt % max(v))
        out("%-26s eval_ms  %s | after_eval_ms  %s | max_backlog  %s   (min / median / max of %d)" % (
            name, mmm("eval_ms", "%.1f"), mmm("after_eval_ms", "%.2f"), mmm("max_backlog", "%d"), a.runs))
    med = lambda name: statistics.median(s["after_eval_ms"] for s in r[name])
    out("after_eval_ms, median, against the built-in call's: " + ", ".join("%s %.2f" % (name, med(name) / med(runs[-1][0])) for name, _ in runs[:-1]))
    pp.free(); ppf.free()
    ctx.close()


if __name__ == "__main__":
    main()
