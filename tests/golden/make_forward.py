#!/usr/bin/env python3
"""Regenerates tests/golden/forward.json from the oracle (oracle/nova.py through its `primary=` seam, oracle/spartan.py,
oracle/wire.py) for the forward MinRoot step circuit of tests/forward_spec.py: the parameters' digests at t = 1 and t = 5,
and the SHA-256 of the compressed proof on the wire for a chain of 3 steps of 5 rounds.

    python tests/golden/make_forward.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import nova as nv, pasta as o, wire  # noqa: E402
from forward_spec import ForwardMinRootCircuit, chain, oracle_pp  # noqa: E402

H = lambda x: "%064x" % x
out = {"note": "oracle-derived; canonical big-endian hex, NOT Montgomery form"}
out["params"] = {str(t): H(oracle_pp(t).params) for t in (1, 5)}

t, n, seed, i0 = 5, 3, 31, 0
init = o.State(o.rand_fe(seed, 0, o.Q), 0, i0)
states = chain(init, t, n)
z0 = [init.x, init.y, init.i]
pp = oracle_pp(t, nv.CCommit())
sn = None
for k in range(n):
    sn = nv.prove_step(pp, sn, ForwardMinRootCircuit(t, states[k], states[k + 1]), z0)
assert nv.verify(pp, sn, n, z0) == ([states[n].x, states[n].y, states[n].i], [0])
c = nv.compress(pp, sn)
assert nv.verify_compressed(pp, c, n, z0) == ([states[n].x, states[n].y, states[n].i], [0])
snark = wire.encode_compressed_proof(t, pp.params, c)
running = wire.encode_running_proof(t, pp.params, sn, z0)
out["wire_t5_n3"] = {"t": t, "steps": n, "seed": seed, "i0": i0, "params": H(pp.params),
                     "compressed_proof_sha256": hashlib.sha256(snark).hexdigest(), "compressed_proof_len": len(snark),
                     "running_proof_sha256": hashlib.sha256(running).hexdigest(), "running_proof_len": len(running)}
path = os.path.join(HERE, "forward.json")
json.dump(out, open(path, "w"), indent=0)
print("wrote", path, os.path.getsize(path), "bytes")
