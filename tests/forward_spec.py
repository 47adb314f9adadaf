"""The specification of the forward MinRoot step circuit (include/vdf_nova.h VDF_CIRCUIT_MINROOT_FORWARD) as a step
circuit for oracle/nova.py's `primary=` seam, shared by tests/test_forward_host.py and tests/test_gpu_forward.py."""
from oracle import nova as nv, pasta as o


class ForwardMinRootCircuit:
    """(x, y, i) -> ((x + y)^(1/5), x + i, i + 1), t rounds: per round the fifth root is allocated, squared twice and
    tmp2 * x' = x + y enforced; y' is a linear combination; then final_i = i_in + t."""

    def __init__(self, t, inp, result):
        self.t, self.input, self.result = t, inp, result

    def arity(self):
        return 3

    def synthesize(self, cs, z):
        x, y, i_in = z
        s = self.input
        for j in range(self.t):
            if s is not None:
                s = o.minroot_eval(s, 1, o.FIELD_FQ)
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


def chain(initial, t, n):
    """states[k] = the state after k steps of t rounds"""
    states = [initial]
    for _ in range(n):
        states.append(o.minroot_eval(states[-1], t, o.FIELD_FQ))
    return states


def oracle_pp(t, commit=None, family=nv.FAMILY_TRY_AND_INCREMENT):
    return nv.public_params(t, commit, nv.GENS_SEED, family, primary=ForwardMinRootCircuit(t, None, None))
