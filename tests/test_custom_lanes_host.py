"""CPU: custom chains in lanes (include/vdf_nova.h vdf_cs_repeat_lanes, vdf_nova_round_tape_eval_lanes, vdf_nova_walk_tape_eval_lanes,
vdf_nova_custom_chain_lanes_from_checkpoints).  No device:

a. the shape of cs.repeat_lanes is the plain double loop's -- the digest, and every triple of the three matrices in both fields --
   and with one lane it is cs.repeat's;
b. the two host evaluators equal a big-integer model (custom_lanes_spec): per-lane inv all distinct, one lane's counter wrapping
   past 2^64, 0, 1 and p - 1 in the advice; the lanes walk equals `lanes` separate vdf_nova_walk_tape_eval calls over the same trace;
c. everything the headers say is refused is refused with VDF_ERR_BAD_ARG, and a valid call after it succeeds;
d. every new symbol is in the libraries, the headers and the Rust crate."""
import os

import numpy as np
import pytest

from oracle import pasta as o
from custom_lanes_spec import (FL, MAX_LANES, every_op_lanes_chain, lanes_checkpoints, model_run_lanes, model_walk_lanes, walk_at_the_slot_cap,
                               walk_inv_and_j_base, window_walks)
from rounds_spec import F, G, MOD, mont_rows
from walks_spec import every_op_body, every_op_ints, expected_bytes, guarded, minroot_body, tape_ints
from vdf_amd import _lib
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError, WALK_MAX_SLOTS, TAPE_MAX_LANES
from vdf_amd.minroot import nova_lib
from vdf_amd.nova import (CustomChain, RoundBody, record_round_body, record_walk_body, round_tape_eval, round_tape_eval_lanes,
                          shape_digest_custom, shape_export_custom, walk_tape_eval, walk_tape_eval_lanes, FIELD_FP, FIELD_FQ)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 1), (2, 5), (3, 64), (16, 2)]          # (lanes, t)


def refused(f, what=None):
    with pytest.raises(VdfError) as e:
        f()
    assert e.value.code == VDF_ERR_BAD_ARG, str(e.value)
    if what:
        assert what in str(e.value), str(e.value)


# ---- a. the shape --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes,t", CASES)
def test_the_digest_of_repeat_lanes_is_the_plain_double_loops(lanes, t):
    assert TAPE_MAX_LANES == MAX_LANES
    d_rep, sizes_rep = shape_digest_custom(FL(t, lanes, "repeat"))
    d_loop, sizes_loop = shape_digest_custom(FL(t, lanes, "loop"))
    assert d_rep == d_loop and sizes_rep == sizes_loop
    # a wider stride of the advice is no part of the shape
    assert shape_digest_custom(FL(t, lanes, "repeat", lane_stride=t + 4))[0] == d_rep
    if lanes == 1:
        assert d_rep == shape_digest_custom(FL(t, 1, "repeat1"))[0] == shape_digest_custom(F(t, "repeat"))[0]
    else:
        assert d_rep != shape_digest_custom(FL(t, lanes - 1, "repeat"))[0]


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("lanes,t", CASES)
def test_every_triple_of_the_shape_in_both_fields(lanes, t, field):
    rep, loop = shape_export_custom(FL(t, lanes, "repeat", field), field), shape_export_custom(FL(t, lanes, "loop", field), field)
    for (r1, c1, v1), (r2, c2, v2) in zip(rep, loop):
        assert r1.tobytes() == r2.tobytes() and c1.tobytes() == c2.tobytes() and v1.tobytes() == v2.tobytes()
    if lanes == 1:
        one = shape_export_custom(F(t, "repeat", field), field)
        assert all(a.tobytes() == b.tobytes() for x, y in zip(rep, one) for a, b in zip(x, y))


# ---- b. the evaluators -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("gap", [0, 3])
@pytest.mark.parametrize("lanes,t", [(1, 3), (2, 5), (5, 9), (16, 2)])
def test_the_round_evaluator_in_lanes_equals_the_integer_model(lanes, t, gap, field):
    m, stride = MOD[field], t + 1 + gap
    tape = record_round_body(G(t, "repeat", field).body(), field)
    assert (tape.c.n_adv, tape.c.n_inv, tape.c.n_vars) == (3, 1, 5)
    rng = np.random.default_rng(100 * lanes + t + gap + field)
    adv = [int(rng.integers(0, 2**62)) ** 5 % m for _ in range(3 * ((lanes - 1) * stride + t + 1))]
    adv[1], adv[4] = 0, 1                               # u_0 and u_1 of lane 0, and p - 1 as a u of the last lane: variables
    adv[3 * ((lanes - 1) * stride + (1 if lanes > 1 else 2)) + 1] = m - 1
    inv = [(0xABCDEF + 17 * l) ** 3 % m for l in range(lanes)]
    assert len(set(inv)) == lanes
    got = round_tape_eval_lanes(field, tape, t, lanes, mont_rows(inv, m), mont_rows(adv, m), stride)
    want = model_run_lanes(G.variables, adv, 3, t, lanes, stride, inv, 1, m)
    assert tape_ints(got, m) == want and {0, m - 1} <= set(want)
    # ... and `lanes` calls of the single evaluator
    for l in range(lanes):
        one = round_tape_eval(field, tape, t, mont_rows(inv[l:l + 1], m), mont_rows(adv[3 * l * stride:3 * (l * stride + t + 1)], m))
        assert got[5 * t * l:5 * t * (l + 1)].tobytes() == one.tobytes()


def lanes_walk_case(field, steps, lanes, t, every):
    """a window of `steps` steps of `lanes` three-column chains: (tape, inv ints, j_base, start ints, expect ints, kw of the call)"""
    inv, j_base, cps = every_op_lanes_chain(field, t, steps, every, lanes)
    per = t // every
    starts, expect = window_walks(cps, lanes, per, 0, steps)
    kw = dict(walk_stride=every, top=every, group=per, group_stride=t + 1, j_base=j_base, j_group_step=t, heads=True)
    return record_walk_body(every_op_body(field), field), inv, j_base, starts, expect, kw


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("steps,lanes,t,every", [(3, 5, 10, 5), (1, 16, 6, 6), (2, 2, 4, 1), (2, 1, 6, 3)])
def test_the_walk_evaluator_in_lanes_equals_the_integer_model(steps, lanes, t, every, field):
    m = MOD[field]
    tape, inv, j_base, starts, expect, kw = lanes_walk_case(field, steps, lanes, t, every)
    assert len(set(inv)) == lanes and (lanes == 1 or j_base[1] == 2**64 - 12)
    n = steps * lanes * (t // every)
    n_tr = 3 * (steps * lanes * (t + 1) + 1)
    entries, trace, ok = mont_rows(starts, m), guarded(n_tr), np.full(n + 1, -7, dtype="<i4")
    walk_tape_eval_lanes(field, tape, lanes, mont_rows(inv, m), entries, n, every, trace, expect=mont_rows(expect, m), ok=ok, **kw)
    land, tr = list(starts), [None] * n_tr
    model_walk_lanes(every_op_ints, m, 3, lanes, inv, 1, land, n, every, tr, **kw)
    assert tape_ints(entries, m) == land == expect and ok.tolist() == [1] * n + [-7]
    assert trace.tobytes() == expected_bytes(tr, m)
    assert sum(v is not None for v in tr) == 3 * steps * lanes * (t + 1)          # complete traces, every entry once, the guard kept
    if lanes >= 3:                                     # (start_entries places them in three different last entries)
        assert {0, 1, m - 1} <= set(v for v in tr if v is not None)
    if lanes == 1:                                                                 # one lane: the single evaluator's bytes
        e1, t1, ok1 = mont_rows(starts, m), guarded(n_tr), np.full(n + 1, -7, dtype="<i4")
        kw1 = dict(kw, j_base=j_base[0])
        walk_tape_eval(field, tape, mont_rows(inv, m), e1, n, every, t1, expect=mont_rows(expect, m), ok=ok1, **kw1)
        assert e1.tobytes() == entries.tobytes() and t1.tobytes() == trace.tobytes() and ok1.tolist() == ok.tolist()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_the_lanes_walk_equals_separate_walks_over_the_same_trace(field):
    """lane l alone: its walks gathered, the trace pointer moved by l (t + 1) entries, group_stride = lanes (t + 1)"""
    m, steps, lanes, t, every = MOD[field], 3, 5, 10, 5
    tape, inv, j_base, starts, expect, kw = lanes_walk_case(field, steps, lanes, t, every)
    per = t // every
    n, n_tr = steps * lanes * per, 3 * (steps * lanes * (t + 1) + 1)
    entries, trace, ok = mont_rows(starts, m), guarded(n_tr), np.zeros(n, dtype="<i4")
    wrong = list(expect)
    wrong[3 * ((1 * lanes + 3) * per + 1) + 2] ^= 1    # step 1, lane 3, its second walk
    walk_tape_eval_lanes(field, tape, lanes, mont_rows(inv, m), entries, n, every, trace, expect=mont_rows(wrong, m), ok=ok, **kw)
    assert ok.tolist() == [0 if w == (1 * lanes + 3) * per + 1 else 1 for w in range(n)]
    e2, trace2, ok2 = mont_rows(starts, m).reshape(n, 12), guarded(n_tr), np.zeros(n, dtype="<i4")
    for l in range(lanes):
        mine = [w for w in range(n) if (w // per) % lanes == l]
        el, okl = np.ascontiguousarray(e2[mine]).reshape(-1, 4), np.zeros(len(mine), dtype="<i4")
        xl = np.ascontiguousarray(mont_rows(wrong, m).reshape(n, 12)[mine]).reshape(-1, 4)
        walk_tape_eval(field, tape, mont_rows(inv[l:l + 1], m), el, len(mine), every, trace2[3 * l * (t + 1):], walk_stride=every, top=every,
                       group=per, group_stride=lanes * (t + 1), j_base=j_base[l], j_group_step=t, heads=True, expect=xl, ok=okl)
        e2[mine] = el.reshape(-1, 12)
        ok2[mine] = okl
    assert e2.tobytes() == entries.tobytes() and trace2.tobytes() == trace.tobytes() and ok2.tolist() == ok.tolist()


# ---- c. refusals -------------------------------------------------------------------------------------------------------------------
def inv_body(n_inv):
    """a round body that reads its last invariant"""
    return RoundBody(n_inv, 1, 1, lambda cs, j, inv, carry, cur, nxt: [cs.mul(cs.add(carry[0], inv[n_inv - 1]), carry[0])])


def test_the_caps_on_lanes_of_the_round_evaluator():
    m, t = o.Q, 3
    tape = record_round_body(inv_body(1))
    adv = mont_rows(list(range(1, 18 * (t + 1) + 1)), m)
    run = lambda lanes, tp=tape, stride=t + 1: round_tape_eval_lanes(FIELD_FQ, tp, t, lanes, mont_rows(list(range(40)), m), adv, stride)
    refused(lambda: run(0), "lanes")
    run(1)
    refused(lambda: run(MAX_LANES + 1), "lanes")
    run(MAX_LANES)                                     # 16 lanes x 1 invariant: at the cap
    # lanes * n_inv beyond VDF_TAPE_MAX_INV = 16.  17 is prime: it is 17 lanes x 1 (above) or 1 lane x 17 invariants (a tape beyond
    # VDF_TAPE_MAX_INV, below); the smallest products beyond the cap that the other two caps admit are 18 = 9 x 2 = 6 x 3
    two, three = record_round_body(inv_body(2)), record_round_body(inv_body(3))
    run(8, two)
    refused(lambda: run(9, two), "n_inv")
    run(5, three)
    refused(lambda: run(6, three), "n_inv")
    wide = record_round_body(inv_body(16))
    run(1, wide)
    wide.c.n_inv = 17
    refused(lambda: run(1, wide))
    refused(lambda: run(2, tape, t), "lane_stride")    # lane_stride < t + 1
    run(2, tape, t + 1)


def test_the_caps_of_the_walk_evaluator_in_lanes():
    m, na = o.Q, 5
    tape = walk_at_the_slot_cap(na, 2)
    start = mont_rows(list(range(1, 3 * na + 1)), m)
    inv = mont_rows(list(range(1, 40)), m)
    run = lambda lanes, tp=tape, **kw: walk_tape_eval_lanes(FIELD_FQ, tp, lanes, inv, start.copy(), 3, 2, group=1, **kw)
    run(3)                                             # accepted at the cap, three lanes
    run(8)                                             # 8 lanes x 2 invariants = VDF_TAPE_MAX_INV
    refused(lambda: run(9), "n_inv")
    refused(lambda: run(0), "lanes")
    refused(lambda: run(MAX_LANES + 1), "lanes")
    # the single evaluator counts no slot for inv: one slot more still runs there, and is one beyond the cap in lanes
    tape.c.n_slots += 1
    assert tape.c.n_slots + 2 * na == WALK_MAX_SLOTS - 1
    walk_tape_eval(FIELD_FQ, tape, inv, start.copy(), 3, 2, group=1)
    refused(lambda: run(1), "n_inv > VDF_WALK_MAX_SLOTS")
    refused(lambda: run(3), "n_inv > VDF_WALK_MAX_SLOTS")
    tape.c.n_slots -= 1
    got = start.copy()
    walk_tape_eval_lanes(FIELD_FQ, tape, 1, inv, got, 3, 2, group=1)
    want = start.copy()
    walk_tape_eval(FIELD_FQ, tape, inv, want, 3, 2, group=1)
    assert got.tobytes() == want.tobytes() != start.tobytes()


def test_repeat_lanes_refuses_and_the_next_synthesis_succeeds():
    t = 3
    good = shape_digest_custom(FL(t, 2))[0]
    for lanes, what in ((0, "lanes"), (MAX_LANES + 1, "lanes")):
        c = FL(t, 2)
        c.synthesize = lambda cs, z, lanes=lanes, c=c: z[:4] + cs.repeat_lanes(c.body(), t, lanes, [z[5]] * lanes, z[:2] * lanes, None)[:2]
        refused(lambda: shape_digest_custom(c), what)
    refused(lambda: shape_digest_custom(FL(t, 2, lane_stride=t)), "lane_stride")
    # lanes * n_inv beyond the cap (9 x 2), and at it (8 x 2)
    class Wide(FL):
        def body(self):
            return RoundBody(2, 2, 2, lambda cs, j, inv, carry, cur, nxt: self.round(cs, j, inv[1:], carry, cs.alloc_from(nxt[0])))

        def synthesize(self, cs, z):
            L = self.lanes
            xy = [v for l in range(L) for v in z[3 * l:3 * l + 2]]
            inv = [z[3 * l + 2] for l in range(L) for _ in range(2)]
            xy = cs.repeat_lanes(self.body(), self.t, L, inv, xy, None)
            return [v for l in range(L) for v in (xy[2 * l], xy[2 * l + 1], z[3 * l + 2])]
    refused(lambda: shape_digest_custom(Wide(t, 9)), "n_inv")
    assert shape_digest_custom(Wide(t, 8))[0] != good
    assert shape_digest_custom(FL(t, 2))[0] == good


def test_the_chain_constructor_in_lanes():
    field, m, t, every, steps, lanes = FIELD_FQ, o.Q, 10, 5, 3, 3
    tape = record_walk_body(minroot_body(field), field)
    inv, j_base = walk_inv_and_j_base(field, lanes)
    per_lane = steps * (t // every) + 1
    cps = lanes_checkpoints(field, t, steps, every, lanes, per_lane + 2)
    make = lambda L=lanes, stride=per_lane + 2, tp=tape, **kw: CustomChain.lanes_from_checkpoints(field, tp, inv, t, every, steps, L, cps, stride,
                                                                                                  j_base[:L] if 0 < L <= lanes else j_base, **kw)
    refused(lambda: make(0), "lanes")
    refused(lambda: make(MAX_LANES + 1), "lanes")
    refused(lambda: make(stride=per_lane - 1), "lane_stride")
    chain = make()
    assert len(chain) == steps and chain.lanes == lanes and chain.memory() == (0, 0)
    assert chain.host_bytes() == tape.c.n_ops * 4 + tape.c.n_consts * 32 + lanes * tape.c.n_inv * 32 + lanes * per_lane * 2 * 32
    chain.free()
    # the slot cap of the walk in lanes holds for a chain of more lanes than one; one lane keeps the single walk's cap
    wide = walk_at_the_slot_cap(5, 2)
    wide.c.n_slots += 1
    wcps, winv = mont_rows(list(range(1, 5 * 2 * (per_lane + 1))), m), mont_rows([1, 2, 3, 4], m)
    refused(lambda: CustomChain.lanes_from_checkpoints(field, wide, winv, t, every, steps, 2, wcps), "VDF_WALK_MAX_SLOTS")
    CustomChain.lanes_from_checkpoints(field, wide, winv, t, every, steps, 1, wcps).free()
    wide.c.n_slots -= 1
    CustomChain.lanes_from_checkpoints(field, wide, winv, t, every, steps, 2, wcps).free()
    # one lane is the constructor that was there
    one = CustomChain.from_checkpoints(field, tape, inv[:1], t, every, steps, cps)
    assert one.lanes == 1 and one.host_bytes() == tape.c.n_ops * 4 + tape.c.n_consts * 32 + tape.c.n_inv * 32 + per_lane * 2 * 32
    one.free()


# ---- d. exports ------------------------------------------------------------------------------------------------------------------
HIP_SYMBOLS = ["vdf_round_tape_run_lanes", "vdf_round_tape_walk_lanes"]
NOVA_SYMBOLS = ["vdf_cs_repeat_lanes", "vdf_nova_round_tape_eval_lanes", "vdf_nova_walk_tape_eval_lanes", "vdf_nova_pp_repeat_lanes",
                "vdf_nova_custom_chain_lanes_from_checkpoints"]


def test_every_new_symbol_is_exported_declared_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "vdf_hip.h")).read()
    nova_h = open(os.path.join(ROOT, "include", "vdf_nova.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "vdf-hip-sys", "src", "lib.rs")).read()
    for s in HIP_SYMBOLS:
        assert hasattr(_lib.lib, s) and s in _lib.PROTOTYPES and s + "(" in hip_h and "pub fn %s(" % s in rust, s
    for s in NOVA_SYMBOLS:
        assert hasattr(nova_lib, s) and getattr(nova_lib, s).argtypes is not None and s + "(" in nova_h and "pub fn %s(" % s in rust, s
    assert "#define VDF_TAPE_MAX_LANES 16" in hip_h
    assert "chains in lanes" not in nova_h.split("Out of scope for custom chains")[1].split("*/")[0]
