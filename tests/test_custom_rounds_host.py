"""CPU: the repeated-rounds seam of a custom step circuit (include/vdf_nova.h vdf_cs_repeat; the reference's extension point is
its StepCircuit trait, src/nova/proof.rs:79-153).  No device: the shape a `repeat` leaves is the shape of the same circuit
written as a plain loop, the recorded tape's semantics (the host evaluator of the very program the kernel runs) equal a big-int
interpretation of the two test circuits, and everything the header says is refused is refused with VDF_ERR_BAD_ARG before a
single variable is made."""
import numpy as np
import pytest

from oracle import pasta as o
from util import ints
from rounds_spec import F, G, MOD, fe, mont_rows
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.nova import RoundBody, StepCircuit, record_round_body, round_tape_eval, shape_digest_custom, FIELD_FP, FIELD_FQ

# include/vdf_nova.h
MAX_INV, MAX_CARRY, MAX_ADV, MAX_OPS, MAX_CONSTS, MAX_VARS, MAX_LIVE = 16, 8, 8, 128, 24, 64, 24


@pytest.mark.parametrize("circuit", [F, G])
@pytest.mark.parametrize("t", [1, 2, 5, 64])
def test_repeat_leaves_the_shape_of_the_plain_loop(circuit, t):
    assert shape_digest_custom(circuit(t, "repeat")) == shape_digest_custom(circuit(t, "loop"))


def test_the_shape_grows_by_the_bodys_variables_and_constraints():
    (_, s1), (_, s2) = shape_digest_custom(F(1, "repeat")), shape_digest_custom(F(6, "repeat"))
    assert s2[0][0] - s1[0][0] == 5 * 3 and s2[0][1] - s1[0][1] == 5 * 3          # 3 constraints and 3 variables per round
    (_, g1), (_, g2) = shape_digest_custom(G(1, "repeat")), shape_digest_custom(G(3, "repeat"))
    assert g2[0][0] - g1[0][0] == 2 * 4 and g2[0][1] - g1[0][1] == 2 * 5          # 3 products + 1 enforce; 5 variables


def special_advice(n, m, rng):
    """n >= 4 values that include 0, 1 and m - 1, in random places"""
    vals = [0, 1, m - 1] + [int(rng.integers(0, 2**62)) ** 5 % m for _ in range(n - 3)]
    return [vals[k] for k in rng.permutation(n)]


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("t", [1, 2, 5, 65])
@pytest.mark.parametrize("circuit", [F, G])
def test_host_evaluator_equals_the_integer_interpretation(circuit, t, field):
    m = MOD[field]
    rng = np.random.default_rng(1000 * t + field)
    c = circuit(t, "repeat", field)
    tape = record_round_body(c.body(), field)
    assert (tape.c.n_vars, tape.c.n_adv, tape.c.n_inv) == (c.n_vars, c.n_adv, 1)
    adv = special_advice((t + 1) * c.n_adv, m, rng)
    assert {0, 1, m - 1} <= set(adv)
    for inv in ([0x1234567], [m - 1]):
        got = round_tape_eval(field, tape, t, mont_rows(inv, m), mont_rows(adv, m))
        assert [o.from_mont(v, m) for v in ints(got)] == circuit.variables(adv, t, inv, m)


def test_slots_are_reused_and_enforce_costs_the_device_nothing():
    f = record_round_body(F(1, "repeat").body())
    # next[0] loaded once and squared in place of nothing: xn, t1, t2 each written out; x, y, i_in and j never loaded (yn is no variable)
    assert f.c.n_slots <= 3 and f.c.n_cons == 3 and len(f.op_list()) == 6
    assert [op for op, *_ in f.op_list()] == [0, 8, 6, 8, 6, 8]
    g = record_round_body(G(1, "repeat").body())
    assert g.c.n_cons == 4 and g.c.n_slots <= 6


class Probe(StepCircuit):
    """arity 1; synthesize runs `self.use(cs, z)` and records the code of the VdfError it raises"""
    arity = 1

    def __init__(self, use):
        self.use, self.codes, self.vars_before = use, [], None

    def synthesize(self, cs, z):
        try:
            self.use(cs, z)
        except VdfError as e:
            self.codes.append(e.code)
            raise
        return z


def refused(use):
    """the circuit's shape synthesis fails with VDF_ERR_BAD_ARG, and so did the call inside it"""
    c = Probe(use)
    with pytest.raises(VdfError) as e:
        shape_digest_custom(c)
    assert e.value.code == VDF_ERR_BAD_ARG and c.codes == [VDF_ERR_BAD_ARG]


def simple_body(n_inv=0, n_carry=1, n_adv=1, body=None):
    return RoundBody(n_inv, n_carry, n_adv, body or (lambda cs, j, inv, carry, cur, nxt: [cs.mul(carry[0], carry[0])] + carry[1:]))


def test_a_well_formed_repeat_is_accepted():
    digest, sizes = shape_digest_custom(Probe(lambda cs, z: cs.repeat(simple_body(), 3, [], z)))
    base = shape_digest_custom(Probe(lambda cs, z: None))[1]
    assert sizes[0][0] - base[0][0] == 3 and sizes[0][1] - base[0][1] == 3


def test_refusals():
    refused(lambda cs, z: cs.repeat(simple_body(body=lambda c, j, inv, carry, cur, nxt: [c.mul(carry[0], z[0])]), 2, [], z))   # a foreign handle
    refused(lambda cs, z: cs.repeat(simple_body(body=lambda c, j, inv, carry, cur, nxt: [c.mul(carry[0], 12345)]), 2, [], z))
    def value_only_in_enforce(c, j, inv, carry, cur, nxt):
        c.enforce(cur[0], carry[0], carry[0])
        return [c.mul(carry[0], carry[0])]
    refused(lambda cs, z: cs.repeat(simple_body(body=value_only_in_enforce), 2, [], z))
    refused(lambda cs, z: cs.repeat(simple_body(body=lambda c, j, inv, carry, cur, nxt: [c.mul(carry[0], c.add(cur[0], j))]), 2, [], z))
    refused(lambda cs, z: cs.repeat(simple_body(body=lambda c, j, inv, carry, cur, nxt: [c.mul(carry[0], carry[0]), nxt[0]][1:]), 2, [], z))  # value-only carry_out
    refused(lambda cs, z: cs.repeat(simple_body(body=lambda c, j, inv, carry, cur, nxt: [c.alloc(None)]), 2, [], z))          # not recordable

    def twice(cs, z):
        out = cs.repeat(simple_body(), 2, [], z)
        cs.repeat(simple_body(), 2, [], out)
    refused(twice)
    refused(lambda cs, z: cs.repeat(simple_body(), 2, [], [99999]))                      # a bad handle in carry_in
    refused(lambda cs, z: cs.repeat(simple_body(), 0, [], z))                            # t = 0
    refused(lambda cs, z: cs.repeat(simple_body(n_carry=2, n_adv=1), 2, [], [z[0], z[0]]))              # n_carry > n_adv


def chain_body(calls, n_vars=1):
    """a body of exactly `calls` recorded calls, `n_vars` of them variables"""
    def b(c, j, inv, carry, cur, nxt):
        a = carry[0]
        for _ in range(n_vars):
            a = c.mul(a, a)
        for _ in range(calls - n_vars):
            a = c.add(a, j)
        return [a]
    return simple_body(body=b)


def live_body(live):
    """exactly `live` values alive at the peak: a_0 = j, a_k = 2 a_(k-1) all kept, then summed into one variable"""
    def b(c, j, inv, carry, cur, nxt):
        a = [j]
        for _ in range(live - 1):
            a.append(c.add(a[-1], a[-1]))
        s = a[0]
        for x in a[1:]:
            s = c.add(s, x)
        c.alloc_from(s)
        return carry
    return simple_body(body=b)


def consts_body(n):
    def b(c, j, inv, carry, cur, nxt):
        a = carry[0]
        for k in range(n):
            a = c.add(a, c.const(fe(k + 1, o.Q)))
        return [c.mul(a, a)]
    return simple_body(body=b)


def accepted(use):
    shape_digest_custom(Probe(use))


def test_each_cap_holds_and_is_refused_one_beyond():
    accepted(lambda cs, z: cs.repeat(chain_body(MAX_OPS), 1, [], z))
    refused(lambda cs, z: cs.repeat(chain_body(MAX_OPS + 1), 1, [], z))
    accepted(lambda cs, z: cs.repeat(chain_body(MAX_VARS, MAX_VARS), 1, [], z))
    refused(lambda cs, z: cs.repeat(chain_body(MAX_VARS + 1, MAX_VARS + 1), 1, [], z))
    accepted(lambda cs, z: cs.repeat(live_body(MAX_LIVE), 1, [], z))
    assert record_round_body(live_body(MAX_LIVE)).c.n_slots == MAX_LIVE
    refused(lambda cs, z: cs.repeat(live_body(MAX_LIVE + 1), 1, [], z))
    accepted(lambda cs, z: cs.repeat(consts_body(MAX_CONSTS), 1, [], z))
    refused(lambda cs, z: cs.repeat(consts_body(MAX_CONSTS + 1), 1, [], z))
    accepted(lambda cs, z: cs.repeat(simple_body(n_inv=MAX_INV), 1, [z[0]] * MAX_INV, z))
    refused(lambda cs, z: cs.repeat(simple_body(n_inv=MAX_INV + 1), 1, [z[0]] * (MAX_INV + 1), z))
    accepted(lambda cs, z: cs.repeat(simple_body(n_carry=MAX_CARRY, n_adv=MAX_ADV), 1, [], [z[0]] * MAX_CARRY))
    refused(lambda cs, z: cs.repeat(simple_body(n_carry=MAX_CARRY + 1, n_adv=MAX_ADV + 1), 1, [], [z[0]] * (MAX_CARRY + 1)))
    refused(lambda cs, z: cs.repeat(simple_body(n_adv=MAX_ADV + 1), 1, [], z))


def test_a_refused_repeat_has_allocated_nothing():
    """the refusal comes before the first variable: a circuit that swallows it has the shape of one without the call"""
    def swallow(cs, z):
        try:
            cs.repeat(chain_body(MAX_OPS + 1), 3, [], z)
        except VdfError:
            pass
    # the failure flag still fails the circuit: what is compared is the recorder, which must leave no trace of the attempt
    with pytest.raises(VdfError):
        shape_digest_custom(Probe(swallow))
    with pytest.raises(VdfError) as e:
        record_round_body(chain_body(MAX_OPS + 1))
    assert e.value.code == VDF_ERR_BAD_ARG
    t = record_round_body(chain_body(MAX_OPS))
    assert t.c.n_vars == 1 and len(t.op_list()) <= 320


def test_the_evaluator_checks_the_tape_it_is_given():
    tape = record_round_body(F(1, "repeat").body())
    adv = mont_rows([1, 2, 3, 4], o.Q)
    tape.ops[0].a = 7                                     # an advice column the tape does not have
    with pytest.raises(VdfError) as e:
        round_tape_eval(FIELD_FQ, tape, 1, mont_rows([5], o.Q), adv)
    assert e.value.code == VDF_ERR_BAD_ARG
    tape = record_round_body(F(1, "repeat").body())
    tape.ops[2].a = 23                                    # a slot nothing wrote
    with pytest.raises(VdfError):
        round_tape_eval(FIELD_FQ, tape, 1, mont_rows([5], o.Q), adv)
