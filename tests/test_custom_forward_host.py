"""CPU: forward bodies of a custom delay function (include/vdf_nova.h vdf_nova_forward_body_record, vdf_cs_pow,
vdf_nova_forward_tape_eval -- the host restatement of include/vdf_hip.h vdf_round_tape_forward_walk and the reference of the
device path).  No device: the MinRoot forward round recorded as a forward body equals the library's own round and its checkpoint
evaluator byte for byte, a body of every op and six powers equals a big-integer interpretation, the layout (strides, base, every,
the counter, a walk cut into calls) is the header's, the forward tape and the inverse walk tape undo each other, and everything
the headers say is refused is refused with VDF_ERR_BAD_ARG."""
import numpy as np
import pytest

from oracle import pasta as o
from rounds_spec import F, MOD, fe, mont_rows
from walks_spec import GUARD, expected_bytes, guarded, minroot_body, start_entries, tape_ints
from forward_tape_spec import (CP_STRIDE, LAYOUT, LAYOUT_FRONT, LAYOUT_TRACE, TAPE_POW, every_op_exponents, every_op_forward_body,
                               every_op_forward_ints, layout_cp_entries, layout_expected, minroot_forward_body, minroot_forward_ints,
                               model_forward, pow_products, root_exponent)
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError, FORWARD_TAPE_MAX_WORK, WALK_MAX_SLOTS
from vdf_amd.minroot import EvalMode, PallasVDF, State, VestaVDF
from vdf_amd.nova import (RoundBody, StepCircuit, WalkBody, forward_tape_eval, record_forward_body, record_round_body, record_walk_body,
                          round_tape_eval, shape_digest_custom, walk_tape_eval, FIELD_FP, FIELD_FQ)

VDF = {FIELD_FQ: PallasVDF, FIELD_FP: VestaVDF}
# include/vdf_nova.h
MAX_INV, MAX_ADV, MAX_OPS, MAX_CONSTS, MAX_LIVE = 16, 8, 128, 24, 24


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("rounds", [1, 2, 5, 65])
def test_a_minroot_forward_body_equals_the_librarys_round_and_its_checkpoints(rounds, field):
    m, n, i0, step = MOD[field], 3, 0xFEDCBA, 1000
    every = 5 if rounds % 5 == 0 else 1
    K = rounds // every
    tape = record_forward_body(minroot_forward_body(field), field)
    assert (tape.c.n_vars, tape.c.n_adv, tape.c.n_inv, tape.c.n_cons) == (2, 2, 0, 0)
    assert [op for op, *_ in tape.op_list()].count(TAPE_POW) == 1
    assert int.from_bytes(tape.consts[0].tobytes(), "little") == root_exponent(field)          # the exponent: a plain integer
    rng = np.random.default_rng(rounds + field)
    states = [State.from_ints(field, int(rng.integers(1, 2**62)) ** 4, int(rng.integers(0, 2**62)) ** 3, i0 + w * step) for w in range(n)]
    entries = np.frombuffer(b"".join(s.x + s.y for s in states), dtype="<u8").reshape(-1, 4).copy()
    stride, cps = rounds + 3, K + 2
    trace, cp = guarded(2 * (n * stride + 1)), guarded(2 * (n * cps + 1))
    forward_tape_eval(field, tape, None, entries, n, rounds, cp, every, cps, trace, stride, 0, j_base=i0, j_walk_step=step)
    vdf = VDF[field].new_with_mode(EvalMode.LTRAddChainSequential)
    want_tr, want_cp = bytearray(b"\xff" * trace.nbytes), bytearray(b"\xff" * cp.nbytes)
    for w, s0 in enumerate(states):
        s = s0
        for r in range(rounds):
            s = vdf.round(s)
            k = w * stride + r + 1
            want_tr[64 * k:64 * k + 64] = s.x + s.y
        assert entries[2 * w:2 * w + 2].tobytes() == s.x + s.y
        assert s.i == State.from_ints(field, 0, 0, i0 + w * step + rounds).i
        for k, c in enumerate(vdf.eval_checkpoints(s0, rounds, every)):
            if k:
                q = w * cps + k
                want_cp[64 * q:64 * q + 64] = c.x + c.y
    assert trace.tobytes() == bytes(want_tr) and cp.tobytes() == bytes(want_cp)


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("rounds", [1, 5])
def test_a_body_of_every_op_equals_the_integer_interpretation(rounds, field):
    m, n = MOD[field], 4
    tape = record_forward_body(every_op_forward_body(field), field)
    ops = tape.op_list()
    assert {op for op, *_ in ops} == set(range(10))                                # every opcode of the tape, POW among them
    assert any(op == 6 and a == b for op, _, a, b in ops)                          # a squaring among the products
    assert all(b == 0 for op, _, a, b in ops if op == 0)                           # the entry stood on
    exps = [int.from_bytes(tape.consts[b].tobytes(), "little") for op, _, a, b in ops if op == TAPE_POW]
    assert exps == every_op_exponents(m)
    start = start_entries(n, 3, m, np.random.default_rng(field))
    assert {0, 1, m - 1} <= set(start)
    for inv in ([0x1234567], [m - 1]):
        kw = dict(walk_stride=rounds + 2, j_base=2**64 - 3, j_walk_step=1)           # J wraps 2^64 inside the walks
        entries, trace = mont_rows(start, m), guarded(3 * (n * (rounds + 2) + 1))
        forward_tape_eval(field, tape, mont_rows(inv, m), entries, n, rounds, trace=trace, **kw)
        land, tr = list(start), [None] * (trace.shape[0])
        model_forward(every_op_forward_ints, m, 3, inv, land, n, rounds, trace=tr, **kw)
        assert tape_ints(entries, m) == land
        assert trace.tobytes() == expected_bytes(tr, m)


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_powers_of_the_special_values(field):
    """x^E for x in {0, 1, m - 1, 2} and every exponent of the every-op body, one power per column"""
    m = MOD[field]
    for e in every_op_exponents(m) + [2**256 - 1, 3]:
        tape = record_forward_body(WalkBody(0, 4, lambda cs, j, inv, cur: [cs.pow(c, e) for c in cur]), field)
        entries = mont_rows([0, 1, m - 1, 2], m)
        forward_tape_eval(field, tape, None, entries, 1, 1)
        assert tape_ints(entries, m) == [pow(x, e, m) for x in (0, 1, m - 1, 2)], e
    assert pow(0, 0, m) == 1


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("every", [1, 2, 5])
def test_strides_base_every_and_the_counter(every, field):
    m = MOD[field]
    tape = record_forward_body(every_op_forward_body(field), field)
    start, inv, want_tr, want_cp, land = layout_expected(field, every)
    n_cp = layout_cp_entries(every)
    entries, tr, cp = mont_rows(start, m), guarded(3 * LAYOUT_TRACE), guarded(3 * n_cp)
    forward_tape_eval(field, tape, mont_rows(inv, m), entries, checkpoints=cp[3 * LAYOUT_FRONT:], every=every, cp_stride=CP_STRIDE[every],
                      trace=tr[3 * LAYOUT_FRONT:], **LAYOUT)
    assert tape_ints(entries, m) == land
    assert tr.tobytes() == expected_bytes(want_tr, m)                              # guards in front, between and behind the runs
    assert cp.tobytes() == expected_bytes(want_cp, m)
    assert sum(v is not None for v in want_tr) // 3 == 6 * 5
    assert sum(v is not None for v in want_cp) // 3 == 6 * {1: 5, 2: 3, 5: 1}[every]
    # the same walk cut into 3 + 2 rounds
    entries2, tr2, cp2 = mont_rows(start, m), guarded(3 * LAYOUT_TRACE), guarded(3 * n_cp)
    cut = dict(LAYOUT)
    for rounds, base in ((3, 3), (2, 6)):
        cut.update(rounds=rounds, base=base)
        forward_tape_eval(field, tape, mont_rows(inv, m), entries2, checkpoints=cp2[3 * LAYOUT_FRONT:], every=every, cp_stride=CP_STRIDE[every],
                          trace=tr2[3 * LAYOUT_FRONT:], **cut)
    assert entries2.tobytes() == entries.tobytes() and tr2.tobytes() == tr.tobytes() and cp2.tobytes() == cp.tobytes()
    # without a trace and checkpoints only the landings are made
    entries3 = mont_rows(start, m)
    forward_tape_eval(field, tape, mont_rows(inv, m), entries3, **LAYOUT)
    assert entries3.tobytes() == entries.tobytes()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_the_forward_tape_and_the_inverse_walk_tape_undo_each_other(field):
    m, n, rounds, i0 = MOD[field], 5, 7, 0xABCDEF
    fwd, back = record_forward_body(minroot_forward_body(field), field), record_walk_body(minroot_body(field), field)
    start = mont_rows(start_entries(n, 2, m, np.random.default_rng(11 + field)), m)
    entries = start.copy()
    # walk w is a chain of its own whose entry k has the counter i0 + 100 w + k
    forward_tape_eval(field, fwd, None, entries, n, rounds, j_base=i0, j_walk_step=100)
    assert entries.tobytes() != start.tobytes()
    land = tape_ints(start, m)
    model_forward(minroot_forward_ints, m, 2, [], land, n, rounds, j_base=i0, j_walk_step=100)
    assert tape_ints(entries, m) == land                                           # ... and the integers
    ok = np.full(n, -7, dtype="<i4")
    walk_tape_eval(field, back, mont_rows([i0], m), entries, n, rounds, top=rounds, group=1, j_group_step=100, expect=start, ok=ok)
    assert entries.tobytes() == start.tobytes() and ok.tolist() == [1] * n


def refused(f):
    with pytest.raises(VdfError) as e:
        f()
    assert e.value.code == VDF_ERR_BAD_ARG


def body(f, n_inv=0, n_adv=1):
    return WalkBody(n_inv, n_adv, f)


def test_a_power_is_legal_in_a_forward_body_only():
    ok = record_forward_body(body(lambda c, j, inv, cur: [c.pow(cur[0], 5)]))
    assert [op for op, *_ in ok.op_list()] == [0, TAPE_POW, 8] and ok.c.n_slots == 1 and ok.c.n_consts == 1
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: [c.pow(nxt[0], 5)])))                  # a descending body
    refused(lambda: record_round_body(RoundBody(0, 1, 1, lambda cs, j, inv, carry, cur, nx: [cs.mul(cs.pow(carry[0], 5), carry[0])])))

    class Live(StepCircuit):                                                                            # a live vdf_cs
        arity = 1

        def synthesize(self, cs, z):
            self.handle = cs.pow(z[0], 5)
            return [cs.mul(z[0], z[0])]
    live = Live()
    refused(lambda: shape_digest_custom(live))
    assert live.handle == 0
    # a POW in a round tape and in a descending walk tape is a malformed op
    t = record_round_body(F(4, "repeat").body())
    advice = mont_rows(list(range(1, 11)), o.Q)
    round_tape_eval(FIELD_FQ, t, 4, mont_rows([1], o.Q), advice)
    mul = next(i for i, x in enumerate(t.op_list()) if x[0] == 6)
    t.ops[mul].op, t.ops[mul].b = TAPE_POW, 0
    t.c.n_consts = 1
    refused(lambda: round_tape_eval(FIELD_FQ, t, 4, mont_rows([1], o.Q), advice))
    w = record_walk_body(minroot_body(FIELD_FQ))
    mul = next(i for i, x in enumerate(w.op_list()) if x[0] == 6)
    w.ops[mul].op, w.ops[mul].b = TAPE_POW, 0
    w.c.n_consts = 1
    refused(lambda: walk_tape_eval(FIELD_FQ, w, mont_rows([1], o.Q), mont_rows([1, 2], o.Q), 1, 1))


def test_the_recorder_refuses_what_is_not_value_arithmetic():
    ok = record_forward_body(body(lambda c, j, inv, cur: [c.mul(cur[0], j)]))
    assert ok.c.n_cons == 0 and ok.c.n_vars == 1
    refused(lambda: record_forward_body(body(lambda c, j, inv, cur: [c.alloc(None)])))
    refused(lambda: record_forward_body(body(lambda c, j, inv, cur: [c.alloc_from(cur[0])])))
    def enforce(c, j, inv, cur):
        c.enforce(cur[0], cur[0], j)
        return [cur[0]]
    refused(lambda: record_forward_body(body(enforce)))
    def value(c, j, inv, cur):
        c.value(cur[0])
        return [cur[0]]
    refused(lambda: record_forward_body(body(value)))
    def repeat(c, j, inv, cur):
        c.repeat(RoundBody(0, 1, 1, lambda cs, j, inv, carry, cu, nx: [cs.mul(carry[0], carry[0])]), 2, [], [cur[0]])
        return [cur[0]]
    refused(lambda: record_forward_body(body(repeat)))
    refused(lambda: record_forward_body(body(lambda c, j, inv, cur: [c.add(cur[0], 12345)])))            # a foreign handle
    refused(lambda: record_forward_body(body(lambda c, j, inv, cur: [12345])))                           # ... in cur_out
    refused(lambda: record_forward_body(body(lambda c, j, inv, cur: [cur[0] + 1])))                      # the other entry of a round body
    refused(lambda: record_forward_body(body(lambda c, j, inv, cur: [cur[0]], n_adv=0)))
    with pytest.raises(ValueError):
        record_forward_body(body(lambda c, j, inv, cur: [c.pow(cur[0], 2**256)]))
    # passed straight through, and one handle in every column
    t = record_forward_body(body(lambda c, j, inv, cur: [cur[1], cur[1]], n_adv=2))
    assert t.op_list() == [(0, 0, 1, 0), (8, 0, 0, 0), (8, 0, 0, 1)] and t.c.n_slots == 1


def chain(calls):
    def b(c, j, inv, cur):
        a = cur[0]
        for _ in range(calls):
            a = c.pow(a, 3)
        return [a]
    return body(b)


def live(n_live, n_adv=1):
    """exactly n_live values alive at the peak, summed into every column"""
    def b(c, j, inv, cur):
        a = [j]
        for _ in range(n_live - 1):
            a.append(c.add(a[-1], a[-1]))
        s = a[0]
        for x in a[1:]:
            s = c.add(s, x)
        return [s] * n_adv
    return body(b, n_adv=n_adv)


def consts(n_const, n_pow):
    """n_const constants and n_pow exponents: one stored constant each"""
    def b(c, j, inv, cur):
        a = cur[0]
        for k in range(n_const):
            a = c.add(a, c.const(fe(k + 1, o.Q)))
        for k in range(n_pow):
            a = c.pow(a, k + 2)
        return [a]
    return body(b)


def test_each_cap_of_the_recorder_holds_and_is_refused_one_beyond():
    assert record_forward_body(chain(MAX_CONSTS)).c.n_ops == MAX_CONSTS + 2
    refused(lambda: record_forward_body(chain(MAX_CONSTS + 1)))                    # the exponents are stored constants
    def calls(n):
        def b(c, j, inv, cur):
            a = cur[0]
            for _ in range(n):
                a = c.add(a, j)
            return [a]
        return body(b)
    record_forward_body(calls(MAX_OPS))
    refused(lambda: record_forward_body(calls(MAX_OPS + 1)))
    record_forward_body(consts(MAX_CONSTS - 3, 3))
    refused(lambda: record_forward_body(consts(MAX_CONSTS - 3, 4)))
    refused(lambda: record_forward_body(consts(MAX_CONSTS - 2, 3)))
    assert record_forward_body(live(MAX_LIVE)).c.n_slots == MAX_LIVE
    refused(lambda: record_forward_body(live(MAX_LIVE + 1)))
    record_forward_body(body(lambda c, j, inv, cur: [c.add(cur[0], inv[MAX_INV - 1])], n_inv=MAX_INV))
    refused(lambda: record_forward_body(body(lambda c, j, inv, cur: [cur[0]], n_inv=MAX_INV + 1)))
    record_forward_body(body(lambda c, j, inv, cur: cur, n_adv=MAX_ADV))
    refused(lambda: record_forward_body(body(lambda c, j, inv, cur: cur, n_adv=MAX_ADV + 1)))
    # live values + the two entries: VDF_WALK_MAX_SLOTS
    assert record_forward_body(live(WALK_MAX_SLOTS - 2 * 5, n_adv=5)).c.n_slots + 2 * 5 == WALK_MAX_SLOTS
    refused(lambda: record_forward_body(live(WALK_MAX_SLOTS - 2 * 5 + 1, n_adv=5)))      # 23 live values: within VDF_ROUND_MAX_LIVE


def run_small(tape, field=FIELD_FQ, rounds=2, **kw):
    na = tape.c.n_adv
    args = dict(trace=guarded(na * (rounds + 1)), walk_stride=0)
    args.update(kw)
    entries = mont_rows(list(range(1, na + 1)), MOD[field])
    forward_tape_eval(field, tape, mont_rows([5], MOD[field]), entries, 1, rounds, **args)
    return entries, args["trace"]


def test_the_evaluator_refuses_what_the_launcher_refuses():
    fresh = lambda: record_forward_body(every_op_forward_body(FIELD_FQ))
    run_small(fresh())
    ops = fresh().op_list()
    first = {k: next(i for i, x in enumerate(ops) if x[0] == k) for k in range(10)}
    def broken(change):
        t = fresh()
        change(t)
        refused(lambda: run_small(t))
    broken(lambda t: setattr(t.ops[first[0]], "b", 1))                            # ADV of the entry being produced
    broken(lambda t: setattr(t.ops[first[0]], "a", 3))                            # a column the tape does not have
    broken(lambda t: setattr(t.ops[first[4]], "op", 10))                          # no such opcode
    broken(lambda t: setattr(t.ops[first[4]], "a", 23))                           # a slot nothing wrote
    broken(lambda t: setattr(t.ops[first[4]], "dst", 24))                         # a slot beyond the file
    broken(lambda t: setattr(t.ops[first[3]], "a", 8))                            # a constant the tape does not have
    broken(lambda t: setattr(t.ops[first[7]], "b", 8))
    broken(lambda t: setattr(t.ops[first[9]], "b", 8))                            # ... as the exponent of a POW
    broken(lambda t: setattr(t.ops[first[9]], "a", 23))                           # a POW of a slot nothing wrote
    broken(lambda t: setattr(t.ops[first[1]], "a", 1))                            # an invariant beyond n_inv
    broken(lambda t: setattr(t.ops[first[8]], "b", 3))                            # a column beyond n_adv
    broken(lambda t: setattr(t.ops[len(ops) - 1], "b", t.ops[len(ops) - 2].b))    # a column written twice, another never
    broken(lambda t: setattr(t.c, "n_ops", len(ops) - 1))                         # a column never written
    broken(lambda t: setattr(t.c, "n_vars", 2))                                   # n_vars != n_adv
    broken(lambda t: setattr(t.c, "n_slots", 25))                                 # beyond VDF_TAPE_MAX_SLOTS
    assert fresh().c.n_consts == 8
    t = fresh()
    refused(lambda: run_small(t, checkpoints=guarded(3 * 3), every=0, cp_stride=3))      # checkpoints without every
    refused(lambda: forward_tape_eval(7, t, mont_rows([5], o.Q), mont_rows([1, 2, 3], o.Q), 1, 1))
    # n_slots + 2 n_adv: 32 holds, 33 is refused
    wide = record_forward_body(live(WALK_MAX_SLOTS - 2 * 5, n_adv=5))
    run_small(wide)
    wide.c.n_slots += 1                                                           # 23 slots: within VDF_TAPE_MAX_SLOTS
    refused(lambda: run_small(wide))
    # nothing to do: no walk, or no round
    e, tr = run_small(t, rounds=0)
    assert tape_ints(e, o.Q) == [1, 2, 3] and (tr == np.uint64(GUARD)).all()
    forward_tape_eval(FIELD_FQ, t, mont_rows([5], o.Q), np.zeros((0, 4), dtype="<u8"), 0, 3)


def test_the_work_cap_counts_the_products_of_a_power():
    """rounds x products per round <= VDF_FORWARD_TAPE_MAX_WORK, a POW counted as bitlen - 1 squarings and popcount - 1 products:
    exactly at the cap runs (2^20 products on the host), one beyond is refused"""
    def one(e, extra_mul=False):
        def b(c, j, inv, cur):
            p = c.pow(cur[0], e)
            return [c.mul(p, cur[0]) if extra_mul else p]
        return record_forward_body(body(b))
    for e, want in ((0, 1), (1, 1), (2, 1), (3, 2), (2**255, 255), (2**255 - 1, 508), (2**256 - 1, 510)):
        assert pow_products(e) == want
        t = one(e)
        entries = mont_rows([3], o.Q)
        refused(lambda: forward_tape_eval(FIELD_FQ, t, None, entries, 1, FORWARD_TAPE_MAX_WORK // want + 1))
        assert tape_ints(entries, o.Q) == [3]
    t = one(2**255, extra_mul=True)                                                # 255 + 1 = 256 products: 4,096 rounds is the cap
    assert FORWARD_TAPE_MAX_WORK % 256 == 0
    rounds = FORWARD_TAPE_MAX_WORK // 256
    entries = mont_rows([3], o.Q)
    forward_tape_eval(FIELD_FQ, t, None, entries, 1, rounds)
    assert tape_ints(entries, o.Q) == [pow(3, pow(2**255 + 1, rounds, o.Q - 1), o.Q)]
    refused(lambda: forward_tape_eval(FIELD_FQ, t, None, entries, 1, rounds + 1))
    none = record_forward_body(body(lambda c, j, inv, cur: [c.add(cur[0], j)]))    # no product: max(1, 0) per round
    entries = mont_rows([3], o.Q)
    forward_tape_eval(FIELD_FQ, none, None, entries, 1, FORWARD_TAPE_MAX_WORK)
    assert tape_ints(entries, o.Q) == [(3 + FORWARD_TAPE_MAX_WORK * (FORWARD_TAPE_MAX_WORK - 1) // 2) % o.Q]
    refused(lambda: forward_tape_eval(FIELD_FQ, none, None, entries, 1, FORWARD_TAPE_MAX_WORK + 1))
