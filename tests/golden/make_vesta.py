#!/usr/bin/env python3
"""Regenerates tests/golden/vesta.json from the oracle (oracle/nova.py with SIDE_FIELD / SIDE_CURVE exchanged -- G1 = Vesta,
the primary circuit over Fp -- oracle/spartan.py, oracle/wire.py) for the specification circuits of tests/vesta_spec.py: the
parameters' digests at t = 1 and t = 5 for the kinds BOUND, REFERENCE, FORWARD and FORWARD_LANES (2 lanes), and the SHA-256
and length of the compressed proof on the wire for a VestaVDF chain of 3 steps of 2 rounds over the forward circuit.

    python tests/golden/make_vesta.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import nova as nv, pasta as o, wire  # noqa: E402
import vesta_spec as vs  # noqa: E402

FP = o.FIELD_FP
H = lambda x: "%064x" % x
KINDS = {"bound": (vs.BOUND, 1), "reference": (vs.REFERENCE, 1), "forward": (vs.FORWARD, 1), "forward_lanes_2": (vs.LANES, 2)}
out = {"note": "oracle-derived under the swapped orientation (primary circuit over Fp); canonical big-endian hex, NOT Montgomery form"}
with vs.swapped():
    out["params"] = {name: {str(t): H(vs.oracle_pp(FP, kind, t, L).params) for t in (1, 5)} for name, (kind, L) in KINDS.items()}
    t, n, seed, i0 = 2, 3, 31, 0
    init = o.State(o.rand_fe(seed, 0, o.P), 0, i0)
    states = vs.chain(FP, init, t, n)
    z0 = [init.x, init.y, init.i]
    pp = vs.oracle_pp(FP, vs.FORWARD, t, commit=nv.CCommit())
    sn = None
    for k in range(n):
        sn = nv.prove_step(pp, sn, vs.ForwardMinRootCircuit(FP, t, states[k], states[k + 1]), z0)
    assert nv.verify(pp, sn, n, z0) == ([states[n].x, states[n].y, states[n].i], [0])
    c = nv.compress(pp, sn)
    assert nv.verify_compressed(pp, c, n, z0) == ([states[n].x, states[n].y, states[n].i], [0])
    snark = wire.encode_compressed_proof(t, pp.params, c)
out["wire_t2_n3"] = {"t": t, "steps": n, "seed": seed, "i0": i0, "params": H(pp.params),
                     "compressed_proof_sha256": hashlib.sha256(snark).hexdigest(), "compressed_proof_len": len(snark)}
path = os.path.join(HERE, "vesta.json")
json.dump(out, open(path, "w"), indent=0)
print("wrote", path, os.path.getsize(path), "bytes")
