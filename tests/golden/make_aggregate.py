#!/usr/bin/env python3
"""Regenerates tests/golden/aggregate.json from the oracle (oracle/nova.py, oracle/spartan.py, oracle/wire.py) through
tests/aggregate_spec.py: the reference's step circuit at t = 2, one chain of three steps walked back from a fixed z0, its running
proofs after 1, 2 and 3 steps, and the aggregates of the first K = 1, 2, 3 of them ("vdf-aggregate-v1", include/vdf_nova.h).

The 1-step proof is there on purpose: its E is zero and its comm_E the identity -- 32 zero bytes on the wire, and the identity
in the point folds.  Committed: length and SHA-256 of every aggregate's bytes, and for the product's host-only verifier fold
(vdf_nova_aggregate_fold_instances) the instances, cross-term commitments, challenges and folded instances of each side.

    python tests/golden/make_aggregate.py         (CPU only; a few minutes: the oracle's arguments are pure Python)
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import nova as nv, pasta as o  # noqa: E402
import aggregate_spec as ag  # noqa: E402

H = lambda x: "%064x" % x
T, STEPS, X0 = 2, 3, 0x5EED


def scenario():
    """(pp, [running proof after 1, 2, 3 steps], entries) -- entry n - 1: (num_steps, z0, zi) of the n-step proof."""
    pp = nv.public_params(T, nv.CCommit(), nv.GENS_SEED, nv.FAMILY_TRY_AND_INCREMENT, bound=False)
    states = [o.State(X0, 0, 0)]
    for _ in range(STEPS):
        states.append(o.minroot_eval(states[-1], T, o.FIELD_FQ))
    z0 = [states[STEPS].x, states[STEPS].y, states[STEPS].i]
    proofs, sn = [], None
    for k in range(STEPS):
        sn = nv.prove_step(pp, sn, nv.InverseMinRootCircuit(T, states[STEPS - k], states[STEPS - k - 1], False), z0)
        proofs.append(sn)
    entries = [(n, z0, [states[STEPS - n].x, states[STEPS - n].y, states[STEPS - n].i]) for n in range(1, STEPS + 1)]
    for sn, (n, a, b) in zip(proofs, entries):
        assert nv.verify(pp, sn, n, a) == (b, [0])
    return pp, proofs, entries


def inst_json(U):
    return {"comm_W": [H(v) for v in U.comm_W], "comm_E": [H(v) for v in U.comm_E], "u": H(U.u), "X": [H(v) for v in U.X]}


def main():
    pp, proofs, entries = scenario()
    assert proofs[0].r[0].comm_E == (0, 0) and not any(proofs[0].r[0].E)
    out = {"note": "oracle-derived; canonical big-endian hex, NOT Montgomery form", "t": T, "x0": H(X0), "params": H(pp.params),
           "entries": [{"num_steps": n, "z0": [H(v) for v in a], "zi": [H(v) for v in b]} for n, a, b in entries], "aggregates": {}}
    digest = int(pp.params).to_bytes(32, "little")
    for K in (1, 2, 3):
        agg = ag.aggregate(pp, proofs[:K])
        ok = ag.verify_aggregate(pp, agg, [e[0] for e in entries[:K]], [e[1] for e in entries[:K]], [e[2] for e in entries[:K]])
        assert ok == (True, -1), ok
        data = ag.encode(T, pp.params, agg)
        assert ag.decode(data, T, pp.params, 3, pp.shapes) == agg
        sides = []
        for side in (0, 1):
            # the instances the verifier folds on this side: R1_k, and its own fold of the secondary pair
            if side == 0:
                insts = [c.r_U1 for c in agg.statements]
            else:
                insts = [nv.nifs_fold(pp, 1, s.r[1], s.l2)[0] for s in proofs[:K]]
            acc, rs = ag.fold_instances(nv.SIDE_FIELD[0], side, digest, insts, agg.comm_TT[side])
            assert rs == agg.trace["r"][side] and acc == agg.trace["acc"][side]
            sides.append({"instances": [inst_json(U) for U in insts], "comm_TT": [[H(v) for v in p] for p in agg.comm_TT[side]],
                          "r": [H(r) for r in rs], "acc": inst_json(acc)})
        out["aggregates"][str(K)] = {"len": len(data), "sha256": hashlib.sha256(data).hexdigest(), "sides": sides}
        print("K =", K, len(data), "bytes", flush=True)
    path = os.path.join(HERE, "aggregate.json")
    json.dump(out, open(path, "w"), indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
