"""CPU: powers by a caller-supplied addition chain (include/vdf_hip.h vdf_pow_step, VDF_TAPE_POWC; include/vdf_nova.h
vdf_cs_pow_chain, vdf_nova_pow_chain_exponent, vdf_nova_pow_chain_window, vdf_minroot_pow_chain; the host evaluator
vdf_nova_forward_tape_eval).  No device.  The oracle throughout: a POWC of a chain with exponent E is byte for byte a POW of E."""
import numpy as np
import pytest

from oracle import pasta as o
from rounds_spec import F, MOD, fe, mont_rows
from walks_spec import expected_bytes, guarded, minroot_body, start_entries, tape_ints
from forward_tape_spec import TAPE_POW, minroot_forward_body, model_forward, root_exponent
from pow_chain_spec import (ACC, NONE, MAX_STEPS, MAX_TMP, TAPE_POWC, EVERY_OP_CHAINS_A, EVERY_OP_CHAINS_B, cases, chain_exponent,
                            chain_products, chain_tmp, every_op_chain_body, every_op_chain_ints, minroot_chain_body, packed_consts,
                            run_chain, tmp_chain, window_chain)
from vdf_amd._lib import VDF_ERR_BAD_ARG, VDF_ERR_BAD_LENGTH
from vdf_amd.hip import VdfError, FORWARD_TAPE_MAX_WORK, WALK_MAX_SLOTS
from vdf_amd import minroot
from vdf_amd.minroot import EvalMode, PallasVDF, State, VestaVDF
from vdf_amd.nova import (RoundBody, StepCircuit, WalkBody, forward_tape_eval, pow_chain_exponent, pow_chain_window, record_forward_body,
                          record_round_body, record_walk_body, round_tape_eval, shape_digest_custom, walk_tape_eval, FIELD_FP, FIELD_FQ)

VDF = {FIELD_FQ: PallasVDF, FIELD_FP: VestaVDF}
FIELDS = [FIELD_FQ, FIELD_FP]


def refused(f, code=VDF_ERR_BAD_ARG):
    with pytest.raises(VdfError) as e:
        f()
    assert e.value.code == code


# ---- the integer model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_every_chain_of_the_tests_is_the_power_by_its_exponent(field):
    m = MOD[field]
    chains = dict(cases(field), minroot=minroot.pow_chain(field))
    for name, steps in chains.items():
        E = chain_exponent(steps)
        assert 1 <= E < 2**256, name
        for x in (0, 1, m - 1, 2, 0x123456789ABCDEF ** 3 % m):
            value, e = run_chain(steps, x, m)
            assert e == E and value == pow(x, E, m), name
        assert pow_chain_exponent(steps) == (E, chain_tmp(steps), chain_products(steps)), name


# ---- the library's own chains -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_the_minroot_chains(field):
    m, steps = MOD[field], minroot.pow_chain(field)
    E, n_tmp, products = pow_chain_exponent(steps)
    assert E == pow(5, -1, m - 1) == root_exponent(field)
    assert len(steps) == 32 and n_tmp == 9
    assert sum(s[1] for s in steps) == 253
    assert sum(1 for s in steps if s[2] != NONE) == {FIELD_FQ: 30, FIELD_FP: 29}[field]
    assert products == 253 + {FIELD_FQ: 30, FIELD_FP: 29}[field]
    assert steps[-1] == (ACC, 0, NONE, NONE) or field == FIELD_FQ          # Fp's 31 steps are padded with one that does nothing
    with pytest.raises(ValueError):
        minroot.pow_chain(7)


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def window_exponents():
    rng = np.random.default_rng(2024)
    rand = [int.from_bytes(rng.bytes(32), "little") >> int(rng.integers(0, 200)) or 1 for _ in range(20)]
    return [1, 2, 3, 2**255, 2**255 - 1, 2**256 - 1, root_exponent(FIELD_FQ), root_exponent(FIELD_FP), o.Q - 2, o.P - 2] + rand


@pytest.mark.parametrize("window", [2, 3, 4])
def test_the_window_generator(window):
    made = 0
    for e in window_exponents():
        want = window_chain(e, window)
        if len(want) > MAX_STEPS:                              # a dense exponent at a small window
            refused(lambda: pow_chain_window(e, window), VDF_ERR_BAD_LENGTH)
            continue
        got = pow_chain_window(e, window)
        assert got == want, hex(e)
        E, n_tmp, products = pow_chain_exponent(got)
        assert E == e and n_tmp == 2**(window - 1) + 1 and products == chain_products(want)
        # a cap one step short, and the cap exactly
        refused(lambda: pow_chain_window(e, window, cap=len(want) - 1), VDF_ERR_BAD_LENGTH)
        assert pow_chain_window(e, window, cap=len(want)) == want
        made += 1
    assert made >= 20
    if window == 2:
        assert len(window_chain(2**256 - 1, 2)) > MAX_STEPS    # ... so that the refusal above is exercised
    if window == 4:
        for field in FIELDS:                                    # 252 squarings, 56 products, 8 for the table
            assert chain_products(window_chain(root_exponent(field), 4)) == 316


def test_the_window_generator_refuses():
    refused(lambda: pow_chain_window(0, 4))
    refused(lambda: pow_chain_window(5, 1))
    refused(lambda: pow_chain_window(5, 5))
    assert pow_chain_window(5, 2) == window_chain(5, 2)
    with pytest.raises(ValueError):
        pow_chain_window(2**256, 4)


# ---- validation -------------------------------------------------------------------------------------------------------------------
def invalid_chains():
    """(name, steps): each invalid for one reason"""
    return [
        ("step 0 from ACC", [(ACC, 1, NONE, NONE)]),
        ("a temporary read before it is written", [(0, 1, NONE, 1), (2, 0, NONE, NONE)]),
        ("a product by a temporary nothing wrote", [(0, 1, 1, NONE)]),
        ("an index equal to the largest n_tmp", [(0, 1, NONE, MAX_TMP)]),
        ("no step", []),
        ("96 steps", [(0, 0, NONE, NONE)] * (MAX_STEPS + 1)),
        ("an exponent reaching 2^256 by squarings", [(0, 255, NONE, 1), (ACC, 1, NONE, NONE)]),
        ("an exponent reaching 2^256 by a product", [(0, 255, NONE, 1), (ACC, 0, 1, NONE)]),
    ]


def test_chain_validation():
    ok = [(0, 1, NONE, NONE)]
    for name, steps in invalid_chains():
        with pytest.raises(VdfError) as e:
            pow_chain_exponent(steps)
        assert e.value.code == VDF_ERR_BAD_ARG, name
        assert pow_chain_exponent(ok) == (2, 1, 1)                                 # a valid call right after it
    assert "step 1" in str(_error(lambda: pow_chain_exponent([(0, 1, NONE, 1), (2, 0, NONE, NONE)])))      # the message names the step
    # the bounds themselves are accepted
    assert pow_chain_exponent(tmp_chain(MAX_TMP)) == (4, MAX_TMP, 2)
    assert pow_chain_exponent([(0, 0, NONE, NONE)] * MAX_STEPS) == (1, 1, 1)       # 95 steps that do nothing: x^1, max(1, 0) products
    # 2^256 - 1 = 2 (2^255 - 1) + 1 is accepted; one more doubling is not
    top = window_chain(2**255 - 1, 4) + [(ACC, 1, 0, NONE)]
    assert pow_chain_exponent(top)[0] == 2**256 - 1
    refused(lambda: pow_chain_exponent(top[:-1] + [(ACC, 2, 0, NONE)]))
    refused(lambda: pow_chain_exponent(top + [(ACC, 0, 0, NONE)]))                  # 2^256 - 1 + 1


def _error(f):
    with pytest.raises(VdfError) as e:
        f()
    return e.value


def chain_tape(field=FIELD_FQ, steps=None):
    """one column: next = cur ^ E(steps)"""
    steps = steps or tmp_chain(3)
    return record_forward_body(WalkBody(0, 1, lambda c, j, inv, cur: [c.pow_chain(cur[0], steps)]), field)


def run_one(tape, field=FIELD_FQ, x=3, rounds=1):
    entries = mont_rows([x], MOD[field])
    forward_tape_eval(field, tape, None, entries, 1, rounds)
    return tape_ints(entries, MOD[field])[0]


def patch(tape, const, byte, value):
    tape.consts.view(np.uint8).reshape(-1)[32 * const + byte] = value


def test_the_packed_chain_and_what_the_evaluator_refuses_about_it():
    steps = minroot.pow_chain(FIELD_FQ)
    t = chain_tape(steps=steps)
    assert t.op_list() == [(0, 0, 0, 0), (TAPE_POWC, 0, 0, 0), (8, 0, 0, 0)] and t.c.n_consts == 5 == packed_consts(steps)
    raw = t.consts[:5].tobytes()
    assert raw[:4] == bytes([32, 9, 0, 0]) and raw[4:4 + 128] == bytes(v for s in steps for v in s) and not any(raw[132:])
    assert run_one(t) == pow(3, root_exponent(FIELD_FQ), o.Q)
    fresh = lambda: chain_tape(steps=steps)

    def broken(change):
        t = fresh()
        change(t)
        refused(lambda: run_one(t))
        assert run_one(fresh()) == pow(3, root_exponent(FIELD_FQ), o.Q)          # a valid call right after it
    broken(lambda t: patch(t, 0, 4, ACC))                       # step 0 from ACC
    broken(lambda t: patch(t, 0, 4, 1))                         # step 0 reads T[1]: read before it is written
    broken(lambda t: patch(t, 0, 7, 9))                         # dst = n_tmp
    broken(lambda t: patch(t, 0, 1, 13))                        # n_tmp = 13
    broken(lambda t: patch(t, 0, 1, 8))                         # n_tmp below an index the chain uses
    broken(lambda t: patch(t, 0, 1, 0))
    broken(lambda t: patch(t, 0, 0, 0))                         # no step
    broken(lambda t: patch(t, 0, 0, 96))                        # 96 steps
    broken(lambda t: patch(t, 0, 2, 1))                         # bytes 2 and 3
    broken(lambda t: patch(t, 0, 3, 1))
    broken(lambda t: patch(t, 4, 4, 1))                         # non-zero padding: the byte behind the last step
    broken(lambda t: patch(t, 4, 31, 1))                        # ... and the last byte of the last constant
    broken(lambda t: patch(t, 0, 4 + 4 * 11 + 1, 255))          # step 11: 64 -> 255 squarings: the exponent passes 2^256
    broken(lambda t: setattr(t.c, "n_consts", 4))               # the chain runs past n_consts
    broken(lambda t: setattr(t.ops[1], "b", 5))                 # the chain's first constant is not one of the tape's
    broken(lambda t: setattr(t.ops[1], "a", 1))                 # a POWC of a slot nothing wrote
    broken(lambda t: setattr(t.ops[1], "dst", 24))
    # n_tmp = 12 declared over a chain that needs 9 is accepted, and so are 95 steps
    t = fresh()
    patch(t, 0, 1, 12)
    assert run_one(t) == pow(3, root_exponent(FIELD_FQ), o.Q)
    t = chain_tape(steps=[(0, 1, NONE, NONE)] + [(ACC, 0, NONE, NONE)] * 94)
    assert t.c.n_consts == 12 and run_one(t) == 9


# ---- the recorder -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_the_minroot_body_with_a_chain_compiles_to_one_powc(field):
    t = record_forward_body(minroot_chain_body(field, minroot.pow_chain(field)), field)
    ops = [op for op, *_ in t.op_list()]
    assert ops[:4] == [0, 0, 4, TAPE_POWC] and ops.count(TAPE_POWC) == 1 and TAPE_POW not in ops
    assert t.c.n_consts == 5 and (t.c.n_vars, t.c.n_adv, t.c.n_inv, t.c.n_cons) == (2, 2, 0, 0)


def test_a_chain_is_legal_in_a_forward_body_only():
    chain = tmp_chain(2)
    refused(lambda: record_walk_body(WalkBody(0, 1, lambda c, j, inv, nxt: [c.pow_chain(nxt[0], chain)])))           # a descending body
    refused(lambda: record_round_body(RoundBody(0, 1, 1, lambda cs, j, inv, carry, cur, nx: [cs.mul(cs.pow_chain(carry[0], chain), carry[0])])))

    class Live(StepCircuit):                                                                                          # a live vdf_cs
        arity = 1

        def synthesize(self, cs, z):
            self.handle = cs.pow_chain(z[0], chain)
            return [cs.mul(z[0], z[0])]
    live = Live()
    refused(lambda: shape_digest_custom(live))
    assert live.handle == 0
    # an invalid chain sets the failure flag in a forward body too
    for name, steps in invalid_chains():
        refused(lambda: chain_tape(steps=steps or [(ACC, 0, NONE, NONE)]))
        assert run_one(chain_tape()) == 81                                                                           # a valid one right after it
    refused(lambda: record_forward_body(WalkBody(0, 1, lambda c, j, inv, cur: [c.pow_chain(12345, chain)])))         # a foreign handle
    # a POWC patched into a round tape and into a descending walk tape is malformed
    t = record_round_body(F(4, "repeat").body())
    advice = mont_rows(list(range(1, 11)), o.Q)
    round_tape_eval(FIELD_FQ, t, 4, mont_rows([1], o.Q), advice)
    src = chain_tape()
    mul = next(i for i, x in enumerate(t.op_list()) if x[0] == 6)
    t.ops[mul].op, t.ops[mul].b = TAPE_POWC, 0
    t.consts[0] = src.consts[0]
    t.c.n_consts = 1
    refused(lambda: round_tape_eval(FIELD_FQ, t, 4, mont_rows([1], o.Q), advice))
    w = record_walk_body(minroot_body(FIELD_FQ))
    mul = next(i for i, x in enumerate(w.op_list()) if x[0] == 6)
    w.ops[mul].op, w.ops[mul].b = TAPE_POWC, 0
    w.consts[0] = src.consts[0]
    w.c.n_consts = 1
    refused(lambda: walk_tape_eval(FIELD_FQ, w, mont_rows([1], o.Q), mont_rows([1, 2], o.Q), 1, 1))


def test_the_chain_takes_its_constants_under_the_cap():
    """24 constants: two chains of 95 steps are 24; a constant more, or a third chain, is one beyond"""
    long = [(0, 1, NONE, NONE)] + [(ACC, 0, NONE, NONE)] * 94

    def b(n_chains, n_consts):
        def f(c, j, inv, cur):
            a = cur[0]
            for _ in range(n_chains):
                a = c.pow_chain(a, long)
            for k in range(n_consts):
                a = c.add(a, c.const(fe(k + 1, o.Q)))
            return [a]
        return WalkBody(0, 1, f)
    assert record_forward_body(b(2, 0)).c.n_consts == 24
    refused(lambda: record_forward_body(b(2, 1)))
    refused(lambda: record_forward_body(b(3, 0)))
    assert record_forward_body(b(1, 12)).c.n_consts == 24


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("rounds", [1, 2, 5, 65])
def test_the_minroot_tape_by_chains_equals_the_pow_tape_and_the_library(rounds, field):
    m, n, i0, step = MOD[field], 3, 0xFEDCBA, 1000
    every = 5 if rounds % 5 == 0 else 1
    K, stride, cps = rounds // every, rounds + 3, rounds // every + 2
    rng = np.random.default_rng(rounds + field)
    states = [State.from_ints(field, int(rng.integers(1, 2**62)) ** 4, int(rng.integers(0, 2**62)) ** 3, i0 + w * step) for w in range(n)]
    states[0] = State.from_ints(field, 5, m - 5, i0)                              # x + y = 0: the root of zero
    start = np.frombuffer(b"".join(s.x + s.y for s in states), dtype="<u8").reshape(-1, 4).copy()

    def run(tape):
        entries, trace, cp = start.copy(), guarded(2 * (n * stride + 1)), guarded(2 * (n * cps + 1))
        forward_tape_eval(field, tape, None, entries, n, rounds, cp, every, cps, trace, stride, 0, j_base=i0, j_walk_step=step)
        return entries.tobytes(), trace.tobytes(), cp.tobytes()
    want = run(record_forward_body(minroot_forward_body(field), field))           # the POW tape
    e = root_exponent(field)
    for steps in (minroot.pow_chain(field), pow_chain_window(e, 4), pow_chain_window(e, 3)):
        assert run(record_forward_body(minroot_chain_body(field, steps), field)) == want
    # ... and the library's own checkpoints
    vdf = VDF[field].new_with_mode(EvalMode.LTRAddChainSequential)
    cp = np.frombuffer(want[2], dtype="<u8").reshape(-1, 8)
    for w, s0 in enumerate(states):
        for k, c in enumerate(vdf.eval_checkpoints(s0, rounds, every)):
            if k:
                assert cp[w * cps + k].tobytes() == c.x + c.y
        assert want[0][64 * w:64 * w + 64] == cp[w * cps + K].tobytes()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("chains", [EVERY_OP_CHAINS_A, EVERY_OP_CHAINS_B], ids=["A", "B"])
def test_a_body_of_every_op_with_powers_by_chains_equals_the_integers(chains, field):
    m, n, rounds = MOD[field], 4, 3
    tape = record_forward_body(every_op_chain_body(field, chains), field)
    ops = tape.op_list()
    assert {op for op, *_ in ops} == set(range(11))                                # every opcode, POW and POWC in one tape
    tmps = [int(tape.consts[b].view(np.uint8)[1]) for op, _, a, b in ops if op == TAPE_POWC]
    assert tmps == [2**(w - 1) + 1 for _, w in chains]
    if chains is EVERY_OP_CHAINS_B:
        assert len(set(tmps)) == 2 and tape.c.n_consts == 8 + 12 + 1               # two POWC of different n_tmp; an 88-step chain
    start = start_entries(n, 3, m, np.random.default_rng(field))
    assert {0, 1, m - 1} <= set(start)
    for inv in ([0x1234567], [m - 1]):
        kw = dict(walk_stride=rounds + 2, j_base=2**64 - 2, j_walk_step=1)           # J wraps 2^64 inside the walks
        entries, trace = mont_rows(start, m), guarded(3 * (n * (rounds + 2) + 1))
        forward_tape_eval(field, tape, mont_rows(inv, m), entries, n, rounds, trace=trace, **kw)
        land, tr = list(start), [None] * (trace.shape[0])
        model_forward(every_op_chain_ints(chains), m, 3, inv, land, n, rounds, trace=tr, **kw)
        assert tape_ints(entries, m) == land
        assert trace.tobytes() == expected_bytes(tr, m)


# ---- the caps ---------------------------------------------------------------------------------------------------------------------
def wide_chain_body(n_tmp, na=5, target=21):
    """a forward body of `na` columns with n_slots + 2 na = target and one chain of n_tmp temporaries: (x + j) (2^k - 1), then ^4"""
    def make(live, tmp):
        def b(c, j, inv, cur):
            a = [c.add(cur[0], j)]
            for _ in range(live - 1):
                a.append(c.add(a[-1], a[-1]))
            s = a[0]
            for x in a[1:]:
                s = c.add(s, x)
            return [c.pow_chain(s, tmp_chain(tmp))] * na
        return WalkBody(0, na, b)
    live = next(k for k in range(2, 24) if record_forward_body(make(k, 2)).c.n_slots + 2 * na == target)
    return make(live, n_tmp), live


def test_the_slot_cap_counts_the_temporaries():
    """n_slots + 2 n_adv + n_tmp: 21 + 11 = 32 is accepted, 21 + 12 = 33 refused -- by the recorder and by the evaluator"""
    body, live = wide_chain_body(11)
    t = record_forward_body(body)
    assert t.c.n_slots + 2 * 5 + 11 == WALK_MAX_SLOTS
    entries = mont_rows([3, 0, 0, 0, 0], o.Q)
    forward_tape_eval(FIELD_FQ, t, None, entries, 1, 1, j_base=4)
    assert tape_ints(entries, o.Q) == [pow(7 * (2**live - 1), 4, o.Q)] * 5
    refused(lambda: record_forward_body(wide_chain_body(12)[0]))
    patch(t, 0, 1, 12)                                          # the same tape with n_tmp = 12 declared: 33
    refused(lambda: forward_tape_eval(FIELD_FQ, t, None, mont_rows([3, 0, 0, 0, 0], o.Q), 1, 1))
    patch(t, 0, 1, 11)
    forward_tape_eval(FIELD_FQ, t, None, mont_rows([3, 0, 0, 0, 0], o.Q), 1, 1)


def test_the_work_cap_counts_the_products_of_a_chain():
    """a POWC counts max(1, squarings + steps with a product): 255 + 1 per round, 4,096 rounds are exactly 2^20 products"""
    steps = [(0, 255, 0, NONE)]
    assert pow_chain_exponent(steps) == (2**255 + 1, 1, 256)
    t = chain_tape(steps=steps)
    rounds = FORWARD_TAPE_MAX_WORK // 256
    assert rounds * 256 == FORWARD_TAPE_MAX_WORK
    entries = mont_rows([3], o.Q)
    refused(lambda: forward_tape_eval(FIELD_FQ, t, None, entries, 1, rounds + 1))
    assert tape_ints(entries, o.Q) == [3]
    forward_tape_eval(FIELD_FQ, t, None, entries, 1, rounds)
    assert tape_ints(entries, o.Q) == [pow(3, pow(2**255 + 1, rounds, o.Q - 1), o.Q)]
    # a chain without a product or a squaring counts one
    idle = chain_tape(steps=[(0, 0, NONE, NONE)])
    entries = mont_rows([3], o.Q)
    forward_tape_eval(FIELD_FQ, idle, None, entries, 1, 1000)
    assert tape_ints(entries, o.Q) == [3]
    refused(lambda: forward_tape_eval(FIELD_FQ, idle, None, entries, 1, FORWARD_TAPE_MAX_WORK + 1))
