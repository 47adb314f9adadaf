"""The specification of the forward MinRoot step circuit in lanes (include/vdf_nova.h VDF_CIRCUIT_MINROOT_FORWARD_LANES) as a
step circuit for oracle/nova.py's `primary=` seam, shared by tests/test_lanes_host.py and tests/test_gpu_lanes.py: L forward
circuits of tests/forward_spec.py side by side, z = (x_0, y_0, i_0, x_1, y_1, i_1, ...)."""
from oracle import nova as nv, pasta as o
from forward_spec import ForwardMinRootCircuit, chain


class LanesForwardCircuit:
    """inputs / results: one state per lane (None, None for the blank circuit of the setup, with `lanes` given)."""

    def __init__(self, t, inputs, results, lanes=None):
        self.t = t
        self.lanes = lanes if inputs is None else len(inputs)
        self.inputs = inputs if inputs is not None else [None] * self.lanes
        self.results = results if results is not None else [None] * self.lanes

    def arity(self):
        return 3 * self.lanes

    def synthesize(self, cs, z):
        out = []
        for l in range(self.lanes):
            out += ForwardMinRootCircuit(self.t, self.inputs[l], self.results[l]).synthesize(cs, z[3 * l:3 * l + 3])
        return out

    def output(self, z):
        return [v for r in self.results for v in (r.x, r.y, r.i)]


def oracle_pp(t, L, commit=None, family=nv.FAMILY_TRY_AND_INCREMENT):
    return nv.public_params(t, commit, nv.GENS_SEED, family, primary=LanesForwardCircuit(t, None, None, lanes=L))


def chains(initials, t, n):
    """states[k][l] = lane l after k steps of t rounds"""
    per_lane = [chain(s, t, n) for s in initials]
    return [[per_lane[l][k] for l in range(len(initials))] for k in range(n + 1)]


def flat(states):
    return [v for s in states for v in (s.x, s.y, s.i)]
