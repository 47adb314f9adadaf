"""CPU: walk bodies of a custom step circuit (include/vdf_nova.h vdf_walk_body, vdf_nova_walk_tape_eval -- the host restatement of
include/vdf_hip.h vdf_round_tape_walk and the reference of the device path).  No device: a MinRoot inverse body equals the
library's own inverse round byte for byte, a body of every op equals a big-integer interpretation, the layout (groups, strides,
heads, the counter, a walk cut into calls) is the header's, expect / ok single out the walks a wrong checkpoint touches, and
everything the headers say is refused is refused with VDF_ERR_BAD_ARG."""
import numpy as np
import pytest

from oracle import pasta as o
from rounds_spec import MOD, fe, mont_rows
from walks_spec import (GUARD, LAYOUT, LAYOUT_ENTRIES, LAYOUT_FRONT, every_op_body, every_op_ints, expected_bytes, guarded, layout_expected,
                        minroot_body, model_walk, start_entries, tape_ints)
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError, WALK_MAX_SLOTS, WALK_MAX_WORK
from vdf_amd.minroot import PallasVDF, State, VestaVDF
from vdf_amd.nova import WalkBody, record_walk_body, walk_tape_eval, FIELD_FP, FIELD_FQ

VDF = {FIELD_FQ: PallasVDF, FIELD_FP: VestaVDF}
# include/vdf_nova.h
MAX_INV, MAX_ADV, MAX_OPS, MAX_CONSTS, MAX_LIVE = 16, 8, 128, 24, 24


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("rounds", [1, 2, 5, 65])
def test_a_minroot_inverse_body_equals_the_librarys_inverse_round(rounds, field):
    m, n, stride, inv0 = MOD[field], 3, rounds + 2, 0xFEDCBA
    tape = record_walk_body(minroot_body(field), field)
    assert (tape.c.n_vars, tape.c.n_adv, tape.c.n_inv, tape.c.n_cons) == (2, 2, 1, 0)
    rng = np.random.default_rng(rounds + field)
    # walk w stands on entry w * stride + rounds of its own chain: the state's counter is inv0 + that index
    states = [State.from_ints(field, int(rng.integers(1, 2**62)) ** 4, int(rng.integers(0, 2**62)) ** 3, inv0 + w * stride + rounds) for w in range(n)]
    entries = np.frombuffer(b"".join(s.x + s.y for s in states), dtype="<u8").reshape(-1, 4).copy()
    trace = guarded(2 * (n * stride + 1))
    walk_tape_eval(field, tape, mont_rows([inv0], m), entries, n, rounds, trace, walk_stride=stride, top=rounds)
    want = bytearray(b"\xff" * trace.nbytes)
    for w, s in enumerate(states):
        for r in range(rounds):
            k = w * stride + rounds - r
            want[64 * k:64 * k + 64] = s.x + s.y
            s = VDF[field].inverse_round(s)
        assert entries[2 * w:2 * w + 2].tobytes() == s.x + s.y
        assert s.i == State.from_ints(field, 0, 0, inv0 + w * stride).i
    assert trace.tobytes() == bytes(want)


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("rounds", [1, 5])
def test_a_body_of_every_op_equals_the_integer_interpretation(rounds, field):
    m, n = MOD[field], 4
    tape = record_walk_body(every_op_body(field), field)
    assert {op for op, *_ in tape.op_list()} == set(range(9))                      # every opcode of the tape
    assert any(op == 6 and a == b for op, _, a, b in tape.op_list())               # a squaring among the products
    start = start_entries(n, 3, m, np.random.default_rng(field))
    assert {0, 1, m - 1} <= set(start)
    for inv in ([0x1234567], [m - 1]):
        entries, trace = mont_rows(start, m), guarded(3 * (n * (rounds + 1) + 1))
        walk_tape_eval(field, tape, mont_rows(inv, m), entries, n, rounds, trace, walk_stride=rounds + 1, top=rounds + 1, j_base=2**64 - 3)
        land, tr = list(start), [None] * (trace.shape[0])
        model_walk(every_op_ints, m, 3, inv, land, n, rounds, tr, walk_stride=rounds + 1, top=rounds + 1, j_base=2**64 - 3)
        assert tape_ints(entries, m) == land
        assert trace.tobytes() == expected_bytes(tr, m)


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("heads", [False, True])
def test_groups_strides_heads_and_the_counter(heads, field):
    m = MOD[field]
    tape = record_walk_body(every_op_body(field), field)
    start, inv, want, land = layout_expected(field, heads)
    entries, buf = mont_rows(start, m), guarded(3 * LAYOUT_ENTRIES)
    walk_tape_eval(field, tape, mont_rows(inv, m), entries, trace=buf[3 * LAYOUT_FRONT:], heads=heads, **LAYOUT)
    assert tape_ints(entries, m) == land
    assert buf.tobytes() == expected_bytes(want, m)                                # guards in front, between and behind the groups
    written = sum(v is not None for v in want) // 3
    assert written == 6 * 5 + (3 if heads else 0)
    # the same walk cut into 3 + 2 rounds
    entries2, buf2 = mont_rows(start, m), guarded(3 * LAYOUT_ENTRIES)
    cut = dict(LAYOUT)
    for rounds, top, h in ((3, 5, False), (2, 2, heads)):
        cut.update(rounds=rounds, top=top)
        walk_tape_eval(field, tape, mont_rows(inv, m), entries2, trace=buf2[3 * LAYOUT_FRONT:], heads=h, **cut)
    assert entries2.tobytes() == entries.tobytes() and buf2.tobytes() == buf.tobytes()
    # without a trace only the landings are made
    entries3 = mont_rows(start, m)
    walk_tape_eval(field, tape, mont_rows(inv, m), entries3, **LAYOUT)
    assert entries3.tobytes() == entries.tobytes()


def test_expect_and_ok_single_out_the_walks_a_wrong_checkpoint_touches():
    """a chain of 4 intervals of 5 rounds from its 5 checkpoints; walk w stands on checkpoint w + 1 and must land on checkpoint w"""
    field, m, every, n = FIELD_FQ, MOD[FIELD_FQ], 5, 4
    tape = record_walk_body(every_op_body(field), field)
    inv = [99]
    cps = [start_entries(1, 3, m, np.random.default_rng(3))]
    for k in range(n):                                                            # downwards: checkpoint index n - k - 1 from n - k
        nxt = list(cps[0])
        model_walk(every_op_ints, m, 3, inv, nxt, 1, every, top=every * (n - k))
        cps.insert(0, nxt)
    run = lambda c: walk_tape_eval(field, tape, mont_rows(inv, m), mont_rows(sum(c[1:], []), m), n, every, walk_stride=every, top=every,
                                   expect=mont_rows(sum(c[:-1], []), m), ok=ok)
    ok = np.full(n + 1, -7, dtype="<i4")
    run(cps)
    assert ok.tolist() == [1, 1, 1, 1, -7]
    wrong = [list(c) for c in cps]
    wrong[2][1] ^= 1                                                              # walk 1 starts from it, walk 2 should land on it
    run(wrong)
    assert ok.tolist() == [1, 0, 0, 1, -7]
    with pytest.raises(VdfError) as e:                                            # expect without ok
        walk_tape_eval(field, tape, mont_rows(inv, m), mont_rows(sum(cps[1:], []), m), n, every, expect=mont_rows(sum(cps[:-1], []), m))
    assert e.value.code == VDF_ERR_BAD_ARG


def refused(f):
    with pytest.raises(VdfError) as e:
        f()
    assert e.value.code == VDF_ERR_BAD_ARG


def body(f, n_inv=0, n_adv=1):
    return WalkBody(n_inv, n_adv, f)


def test_the_recorder_refuses_what_is_not_value_arithmetic():
    ok = record_walk_body(body(lambda c, j, inv, nxt: [c.mul(nxt[0], j)]))
    assert ok.c.n_cons == 0 and ok.c.n_vars == 1
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: [c.alloc(None)])))
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: [c.alloc_from(nxt[0])])))
    def enforce(c, j, inv, nxt):
        c.enforce(nxt[0], nxt[0], j)
        return [nxt[0]]
    refused(lambda: record_walk_body(body(enforce)))
    def value(c, j, inv, nxt):
        c.value(nxt[0])
        return [nxt[0]]
    refused(lambda: record_walk_body(body(value)))
    def repeat(c, j, inv, nxt):
        from vdf_amd.nova import RoundBody
        c.repeat(RoundBody(0, 1, 1, lambda cs, j, inv, carry, cur, nx: [cs.mul(carry[0], carry[0])]), 2, [], [nxt[0]])
        return [nxt[0]]
    refused(lambda: record_walk_body(body(repeat)))
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: [c.add(nxt[0], 12345)])))            # a foreign handle
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: [12345])))                           # ... in cur_out
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: [nxt[0] - 1])))                      # the `cur` a round body has: not a walk body's
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: [nxt[0]], n_adv=0)))
    # passed straight through, and one handle in every column
    t = record_walk_body(body(lambda c, j, inv, nxt: [nxt[1], nxt[1]], n_adv=2))
    assert [op for op, *_ in t.op_list()] == [0, 8, 8] and t.c.n_slots == 1


def chain(calls):
    def b(c, j, inv, nxt):
        a = nxt[0]
        for _ in range(calls):
            a = c.add(a, j)
        return [a]
    return body(b)


def live(n_live, n_adv=1):
    """exactly n_live values alive at the peak (live_body of the round tests), summed into column 0"""
    def b(c, j, inv, nxt):
        a = [j]
        for _ in range(n_live - 1):
            a.append(c.add(a[-1], a[-1]))
        s = a[0]
        for x in a[1:]:
            s = c.add(s, x)
        return [s] * n_adv
    return body(b, n_adv=n_adv)


def consts(n):
    def b(c, j, inv, nxt):
        a = nxt[0]
        for k in range(n):
            a = c.add(a, c.const(fe(k + 1, o.Q)))
        return [a]
    return body(b)


def test_each_cap_of_the_recorder_holds_and_is_refused_one_beyond():
    record_walk_body(chain(MAX_OPS))
    refused(lambda: record_walk_body(chain(MAX_OPS + 1)))
    record_walk_body(consts(MAX_CONSTS))
    refused(lambda: record_walk_body(consts(MAX_CONSTS + 1)))
    assert record_walk_body(live(MAX_LIVE)).c.n_slots == MAX_LIVE
    refused(lambda: record_walk_body(live(MAX_LIVE + 1)))
    record_walk_body(body(lambda c, j, inv, nxt: [c.add(nxt[0], inv[MAX_INV - 1])], n_inv=MAX_INV))
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: [nxt[0]], n_inv=MAX_INV + 1)))
    record_walk_body(body(lambda c, j, inv, nxt: nxt, n_adv=MAX_ADV))
    refused(lambda: record_walk_body(body(lambda c, j, inv, nxt: nxt, n_adv=MAX_ADV + 1)))
    # live values + the two entries: VDF_WALK_MAX_SLOTS
    assert record_walk_body(live(WALK_MAX_SLOTS - 2 * 5, n_adv=5)).c.n_slots + 2 * 5 == WALK_MAX_SLOTS
    refused(lambda: record_walk_body(live(WALK_MAX_SLOTS - 2 * 5 + 1, n_adv=5)))         # 23 live values: within VDF_ROUND_MAX_LIVE


def run_small(tape, field=FIELD_FQ, rounds=2, **kw):
    na = tape.c.n_adv
    args = dict(trace=guarded(na * (rounds + 1)), top=rounds)
    args.update(kw)
    entries = mont_rows(list(range(1, na + 1)), MOD[field])
    walk_tape_eval(field, tape, mont_rows([5], MOD[field]), entries, 1, rounds, **args)
    return entries, args["trace"]


def test_the_evaluator_refuses_what_the_launcher_refuses():
    fresh = lambda: record_walk_body(every_op_body(FIELD_FQ))
    run_small(fresh())
    ops = fresh().op_list()
    first = {k: next(i for i, x in enumerate(ops) if x[0] == k) for k in range(9)}
    def broken(change):
        t = fresh()
        change(t)
        refused(lambda: run_small(t))
    broken(lambda t: setattr(t.ops[first[0]], "b", 0))                            # ADV of the entry being produced
    broken(lambda t: setattr(t.ops[first[0]], "a", 3))                            # a column the tape does not have
    broken(lambda t: setattr(t.ops[first[4]], "op", 9))                           # no such opcode
    broken(lambda t: setattr(t.ops[first[4]], "a", 23))                           # a slot nothing wrote
    broken(lambda t: setattr(t.ops[first[4]], "dst", 24))                         # a slot beyond the file
    broken(lambda t: setattr(t.ops[first[3]], "a", 5))                            # a constant the tape does not have
    broken(lambda t: setattr(t.ops[first[7]], "b", 5))
    broken(lambda t: setattr(t.ops[first[1]], "a", 1))                            # an invariant beyond n_inv
    broken(lambda t: setattr(t.ops[first[8]], "b", 3))                            # a column beyond n_adv
    broken(lambda t: setattr(t.ops[len(ops) - 1], "b", t.ops[len(ops) - 2].b))    # a column written twice, another never
    broken(lambda t: setattr(t.c, "n_ops", len(ops) - 1))                         # a column never written
    broken(lambda t: setattr(t.c, "n_vars", 2))                                   # n_vars != n_adv
    broken(lambda t: setattr(t.c, "n_slots", 25))                                 # beyond VDF_TAPE_MAX_SLOTS
    t = fresh()
    refused(lambda: run_small(t, rounds=5, top=3))                                # top < rounds - 1
    run_small(t, rounds=5, top=4, trace=guarded(3 * 5))
    refused(lambda: run_small(t, rounds=5, top=4, trace=guarded(3 * 5), heads=True))      # the landing would be entry -1
    refused(lambda: walk_tape_eval(7, t, mont_rows([5], o.Q), mont_rows([1, 2, 3], o.Q), 1, 1))
    # n_slots + 2 n_adv: 32 holds, 33 is refused
    wide = record_walk_body(live(WALK_MAX_SLOTS - 2 * 5, n_adv=5))
    run_small(wide)
    wide.c.n_slots += 1                                                           # 23 slots: within VDF_TAPE_MAX_SLOTS
    refused(lambda: run_small(wide))
    # work = rounds x products per round (3 here: two MUL, one SCALE): one beyond VDF_WALK_MAX_WORK is refused.  Acceptance AT the
    # cap is not run: it would be seconds of sequential products on the host.
    products = sum(op in (6, 7) for op, *_ in ops)
    assert products == 3
    refused(lambda: run_small(t, rounds=WALK_MAX_WORK // products + 1, trace=None))
    none = record_walk_body(body(lambda c, j, inv, nxt: [c.add(nxt[0], j)]))      # no product: max(1, 0) per round
    refused(lambda: run_small(none, rounds=WALK_MAX_WORK + 1, trace=None))
    # nothing to do: no walk, or no round
    e, tr = run_small(t, rounds=0)
    assert tape_ints(e, o.Q) == [1, 2, 3] and (tr == np.uint64(GUARD)).all()
    walk_tape_eval(FIELD_FQ, t, mont_rows([5], o.Q), np.zeros((0, 4), dtype="<u8"), 0, 3)
