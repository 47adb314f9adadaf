#!/usr/bin/env python3
"""Regenerates tests/golden/lanes.json from the oracle (oracle/nova.py through its `primary=` seam, oracle/spartan.py,
oracle/wire.py) for the forward MinRoot step circuit in lanes of tests/lanes_spec.py: the parameters' digests at
(L, t) = (2, 1), (2, 3), (3, 5), and length and SHA-256 of the compressed and the running proof on the wire for two lanes of
3 steps of 3 rounds.

    python tests/golden/make_lanes.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import nova as nv, pasta as o, wire  # noqa: E402
from lanes_spec import LanesForwardCircuit, chains, flat, oracle_pp  # noqa: E402

H = lambda x: "%064x" % x
out = {"note": "oracle-derived; canonical big-endian hex, NOT Montgomery form"}
out["params"] = {"%d,%d" % (L, t): H(oracle_pp(t, L).params) for L, t in ((2, 1), (2, 3), (3, 5))}

L, t, n, seed, i0 = 2, 3, 3, 41, (0, 5)
inits = [o.State(o.rand_fe(seed, l, o.Q), 0, i0[l]) for l in range(L)]
states = chains(inits, t, n)
z0 = flat(inits)
pp = oracle_pp(t, L, nv.CCommit())
sn = None
for k in range(n):
    sn = nv.prove_step(pp, sn, LanesForwardCircuit(t, states[k], states[k + 1]), z0)
assert nv.verify(pp, sn, n, z0) == (flat(states[n]), [0])
c = nv.compress(pp, sn)
assert nv.verify_compressed(pp, c, n, z0) == (flat(states[n]), [0])
snark = wire.encode_compressed_proof(t, pp.params, c)
running = wire.encode_running_proof(t, pp.params, sn, z0)
out["wire_L2_t3_n3"] = {"lanes": L, "t": t, "steps": n, "seed": seed, "i0": list(i0), "params": H(pp.params),
                        "compressed_proof_sha256": hashlib.sha256(snark).hexdigest(), "compressed_proof_len": len(snark),
                        "running_proof_sha256": hashlib.sha256(running).hexdigest(), "running_proof_len": len(running)}
path = os.path.join(HERE, "lanes.json")
json.dump(out, open(path, "w"), indent=0)
print("wrote", path, os.path.getsize(path), "bytes")
