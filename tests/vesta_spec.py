"""The specification circuits of the cycle in either orientation (include/vdf_nova.h vdf_nova_public_params_field), with the
field as a parameter, for oracle/nova.py's `primary=` seam; shared by tests/test_vesta_host.py and tests/test_gpu_vesta.py.
The oracle takes its orientation from the module-level tuples SIDE_FIELD / SIDE_CURVE: `swapped()` exchanges them for the
length of a `with` block (field FP: G1 = Vesta, G2 = Pallas) and puts them back, because other test files read them."""
import contextlib

import pytest

from oracle import nova as nv, pasta as o


@contextlib.contextmanager
def oriented(field):
    """The oracle in the orientation `field` (the primary circuit's field); FIELD_FQ leaves it as it is."""
    with pytest.MonkeyPatch.context() as mp:
        if field == o.FIELD_FP:
            mp.setattr(nv, "SIDE_FIELD", (o.FIELD_FP, o.FIELD_FQ))
            mp.setattr(nv, "SIDE_CURVE", (o.CURVE_VESTA, o.CURVE_PALLAS))
        yield


def swapped():
    return oriented(o.FIELD_FP)


class ForwardMinRootCircuit:
    """tests/forward_spec.py's circuit over `field`: (x, y, i) -> ((x + y)^(1/5), x + i, i + 1), t rounds."""

    def __init__(self, field, t, inp, result):
        self.field, self.t, self.input, self.result = field, t, inp, result

    def arity(self):
        return 3

    def synthesize(self, cs, z):
        x, y, i_in = z
        s = self.input
        for j in range(self.t):
            if s is not None:
                s = o.minroot_eval(s, 1, self.field)
            nx = cs.alloc(s.x if s is not None else 0)
            t1 = cs.mul(nx, nx)
            t2 = cs.mul(t1, t1)
            cs.enforce(t2, nx, cs.add(x, y))
            y = cs.lin([(1, x), (1, i_in), (j, cs.const(1))])
            x = nx
        fi = cs.alloc((i_in.v + self.t) % cs.m)
        cs.enforce(fi, cs.const(1), cs.add(i_in, cs.const(self.t)))
        return [x, y, fi]

    def output(self, z):
        return [self.result.x, self.result.y, self.result.i]


class LanesForwardCircuit:
    """tests/lanes_spec.py's circuit over `field`: L forward circuits side by side, z = (x_0, y_0, i_0, x_1, ...)."""

    def __init__(self, field, t, inputs, results, lanes=None):
        self.field, self.t = field, t
        self.lanes = lanes if inputs is None else len(inputs)
        self.inputs = inputs if inputs is not None else [None] * self.lanes
        self.results = results if results is not None else [None] * self.lanes

    def arity(self):
        return 3 * self.lanes

    def synthesize(self, cs, z):
        out = []
        for l in range(self.lanes):
            out += ForwardMinRootCircuit(self.field, self.t, self.inputs[l], self.results[l]).synthesize(cs, z[3 * l:3 * l + 3])
        return out

    def output(self, z):
        return [v for r in self.results for v in (r.x, r.y, r.i)]


class CubicCircuit:
    """oracle/nova.py's CubicCircuit with `output` reduced mod the chosen field: arity 1, z -> z^3 + z + 5."""

    def __init__(self, field):
        self.field = field

    def arity(self):
        return 1

    def synthesize(self, cs, z):
        return nv.CubicCircuit().synthesize(cs, z)

    def output(self, z):
        return [(z[0] ** 3 + z[0] + 5) % o.modulus(self.field)]


def chain(field, initial, t, n):
    """states[k] = the state after k steps of t rounds over `field`"""
    states = [initial]
    for _ in range(n):
        states.append(o.minroot_eval(states[-1], t, field))
    return states


def chains(field, initials, t, n):
    """states[k][l] = lane l after k steps of t rounds"""
    per_lane = [chain(field, s, t, n) for s in initials]
    return [[per_lane[l][k] for l in range(len(initials))] for k in range(n + 1)]


def flat(states):
    return [v for s in states for v in (s.x, s.y, s.i)]


# the product's circuit kinds (include/vdf_nova.h)
BOUND, REFERENCE, FORWARD, LANES = 0, 1, 3, 4


def blank_primary(field, kind, t, lanes=1):
    """the blank primary step circuit of `kind` for nv.public_params(primary=...); None: the oracle's own inverse circuit"""
    if kind == FORWARD or (kind == LANES and lanes == 1):
        return ForwardMinRootCircuit(field, t, None, None)
    if kind == LANES:
        return LanesForwardCircuit(field, t, None, None, lanes=lanes)
    return None


def oracle_pp(field, kind, t, lanes=1, commit=None, family=nv.FAMILY_TRY_AND_INCREMENT):
    """The oracle's parameters in the orientation `field`; call under `oriented(field)`."""
    assert nv.SIDE_FIELD[0] == field, "call under vesta_spec.oriented(field)"
    return nv.public_params(t, commit, nv.GENS_SEED, family, bound=(kind == BOUND), primary=blank_primary(field, kind, t, lanes))
