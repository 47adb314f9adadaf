"""CPU: the chain of a custom step circuit (include/vdf_nova.h vdf_custom_chain) without a device -- the constructor's refusals,
its accounting, vdf_cs_step_advice while a shape is recorded, the exports, and the rule by which materialize cuts the walks of a
window into launches, run through the library's own arithmetic over the host restatement of the walk."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from custom_chain_spec import FC, checkpoints_of, every_op_chain, minroot_chain, model_window
from rounds_spec import F, MOD, mont_rows
from walks_spec import every_op_body, every_op_ints, expected_bytes, minroot_body, minroot_ints
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.minroot import nova_lib
from vdf_amd.nova import (CustomChain, WalkBody, custom_chain_slices, custom_chain_window_host, record_forward_body, record_walk_body,
                          shape_digest_custom, shape_export_custom, FIELD_FP, FIELD_FQ)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vdf_nova_custom_chain_from_checkpoints", "vdf_nova_custom_chain_materialize", "vdf_nova_custom_chain_release",
       "vdf_nova_custom_chain_memory", "vdf_nova_custom_chain_host_bytes", "vdf_nova_custom_chain_len", "vdf_nova_custom_chain_advice",
       "vdf_nova_custom_chain_free", "vdf_nova_custom_chain_slice", "vdf_cs_step_advice", "vdf_nova_prove_step_custom_chain",
       "vdf_nova_prove_recursively_custom", "vdf_nova_proof_last_unsat", "vdf_nova_pp_repeat_rows"]


def good(field=FIELD_FQ, t=65, every=13, steps=7):
    m = MOD[field]
    tape = record_walk_body(minroot_body(field), field)
    cps = checkpoints_of(minroot_chain(field, t, steps), 2, every, m)
    return tape, mont_rows([7], m), cps


def refused(what, field=FIELD_FQ, tape=None, inv="good", t=65, every=13, steps=7, cps="good"):
    g_tape, g_inv, g_cps = good()
    with pytest.raises(VdfError) as e:
        CustomChain.from_checkpoints(field, tape or g_tape, g_inv if isinstance(inv, str) else inv, t, every, steps,
                                     g_cps if isinstance(cps, str) else cps)
    assert e.value.code == VDF_ERR_BAD_ARG
    assert what in str(e.value), str(e.value)


def test_every_refusal_of_the_constructor_and_a_valid_chain_right_after():
    fresh = lambda: record_walk_body(minroot_body(FIELD_FQ), FIELD_FQ)
    t = fresh()
    t.ops[0].op = 200
    refused("malformed", tape=t)                                   # a malformed op
    t = fresh()
    t.c.n_vars = 1
    refused("n_vars != n_adv", tape=t)
    t = fresh()
    adv = next(i for i, x in enumerate(t.op_list()) if x[0] == 0)
    t.ops[adv].b = 0
    refused("malformed", tape=t)                                   # an ADV of the entry being produced
    fwd = record_forward_body(WalkBody(0, 1, lambda cs, j, inv, nxt: [cs.pow(nxt[0], 5)]), FIELD_FQ)
    refused("malformed", tape=fwd)                                 # a POW (and its ADV with b = 0)
    def wide(c, j, inv, nxt):                                      # 22 values alive at once, five columns: 22 + 2 * 5 = 32 slots
        a = [c.add(nxt[0], j)]
        for _ in range(21):
            a.append(c.add(a[-1], a[-1]))
        s = a[0]
        for x in a[1:]:
            s = c.add(s, x)
        return [s] * 5
    t = record_walk_body(WalkBody(0, 5, wide), FIELD_FQ)
    assert t.c.n_slots + 10 == 32
    big = np.zeros(((7 * 5 + 1) * 5, 4), dtype="<u8")
    CustomChain.from_checkpoints(FIELD_FQ, t, None, 65, 13, 7, big).free()
    t.c.n_slots += 1
    refused("VDF_WALK_MAX_SLOTS", tape=t, cps=big)                 # one slot beyond the cap
    refused("`every`", every=0)
    refused("`every`", every=12)                                   # 65 = 5 * 13
    refused("num_steps", steps=0)
    refused("field", field=5)
    refused("t out of range", t=0, every=1)
    # null pointers, through the C ABI itself
    g_tape, g_inv, g_cps = good()
    h = C.c_void_p()
    call = nova_lib.vdf_nova_custom_chain_from_checkpoints
    for args in ((FIELD_FQ, None, g_inv.ctypes.data, 65, 13, 7, g_cps.ctypes.data, 0, C.byref(h)),
                 (FIELD_FQ, C.addressof(g_tape.c), None, 65, 13, 7, g_cps.ctypes.data, 0, C.byref(h)),
                 (FIELD_FQ, C.addressof(g_tape.c), g_inv.ctypes.data, 65, 13, 7, None, 0, C.byref(h)),
                 (FIELD_FQ, C.addressof(g_tape.c), g_inv.ctypes.data, 65, 13, 7, g_cps.ctypes.data, 0, None)):
        assert call(*args) == VDF_ERR_BAD_ARG and b"null" in nova_lib.vdf_nova_last_error() and not h.value
    chain = CustomChain.from_checkpoints(FIELD_FQ, g_tape, g_inv, 65, 13, 7, g_cps)
    assert len(chain) == 7
    chain.free()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_len_host_bytes_and_memory(field):
    tape, inv, cps = good(field)
    chain = CustomChain.from_checkpoints(field, tape, inv, 65, 13, 7, cps, j_base=2**64 - 5)
    assert len(chain) == 7
    assert cps.shape[0] == (7 * 5 + 1) * 2
    assert chain.host_bytes() == tape.c.n_ops * 4 + tape.c.n_consts * 32 + tape.c.n_inv * 32 + cps.nbytes
    assert chain.memory() == (0, 0)
    chain.free()
    assert nova_lib.vdf_nova_custom_chain_len(None) == 0


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_step_advice_is_null_while_a_shape_is_recorded_and_changes_no_shape(field):
    t = 5
    c, plain = FC(t, field), F(t, "repeat", field)
    got, want = shape_export_custom(c, field), shape_export_custom(plain, field)
    assert c.seen and all(s == (False, None) for s in c.seen)
    assert repr(got) == repr(want) or all(np.array_equal(a, b) for x, y in zip(got, want) for a, b in zip(x, y))
    if field == FIELD_FQ:
        c.seen.clear()
        assert shape_digest_custom(c) == shape_digest_custom(plain)
        assert c.seen and all(s == (False, None) for s in c.seen)


def test_every_new_symbol_is_exported_and_declared():
    import vdf_amd.nova                                           # noqa: F401  (sets its prototypes on import)
    from vdf_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdf_nova.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "vdf-hip-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert hasattr(nova_lib, name) and getattr(nova_lib, name).argtypes is not None, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert "pub fn %s(" % name in rust, name
    assert "VDF_CUSTOM_CHECK_STEPS" in header
    hip = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdf_hip.h")).read(), flags=re.S)
    for name in ("vdf_unsat_rows", "vdf_ptr_download"):
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES and re.search(r"\b%s\s*\(" % name, hip) and "pub fn %s(" % name in rust


@pytest.mark.parametrize("every,launch_rounds", [(13, 4), (13, 13), (13, 100), (1, 1), (5, 2)])
def test_the_slices_of_a_window_equal_one_uncut_call(every, launch_rounds):
    """materialize's sequence of walk calls (vdf_nova_custom_chain_slice) against ONE call of `every` rounds, both over the host
    restatement: trace, landings and ok byte for byte; and against the big-integer model of the window"""
    field, steps, first, count, j_base = FIELD_FQ, 4, 1, 3, 2**64 - 70
    t = 5 * every
    m = MOD[field]
    tape = record_walk_body(every_op_body(field), field)
    inv, cp_ints = every_op_chain(field, t, steps, every, j_base)
    cps = mont_rows(cp_ints, m)
    slices = custom_chain_slices(every, launch_rounds)
    assert sum(s[0] for s in slices) == every and [s[2] for s in slices] == [False] * (len(slices) - 1) + [True]
    assert all(r <= launch_rounds and top >= r for r, top, _ in slices) and slices[0][1] == every
    trace, land, ok = custom_chain_window_host(field, tape, mont_rows(inv, m), t, every, cps, first, count, j_base, launch_rounds)
    trace1, land1, ok1 = custom_chain_window_host(field, tape, mont_rows(inv, m), t, every, cps, first, count, j_base, every)
    assert len(custom_chain_slices(every, every)) == 1
    assert trace.tobytes() == trace1.tobytes() and land.tobytes() == land1.tobytes() and ok.tobytes() == ok1.tobytes()
    assert ok.tolist() == [1] * (count * 5)
    want, good_steps = model_window(every_op_ints, m, 3, inv, cp_ints, first, count, t, every, j_base)
    assert None not in want and good_steps == [True] * count
    assert trace.tobytes() == expected_bytes(want, m)


def test_the_default_launch_length_and_the_refusals_of_the_slice():
    assert custom_chain_slices(2500) == [(1024, 2500, False), (1024, 1476, False), (452, 452, True)]
    r, top, last = C.c_uint64(), C.c_uint64(), C.c_int()
    call = nova_lib.vdf_nova_custom_chain_slice
    assert call(13, 4, 8, 3, C.byref(r), C.byref(top), C.byref(last)) == 0 and (r.value, top.value, last.value) == (3, 5, 0)   # a pump's budget
    assert call(13, 4, 12, 3, C.byref(r), C.byref(top), C.byref(last)) == 0 and (r.value, top.value, last.value) == (1, 1, 1)
    assert call(0, 4, 0, 0, C.byref(r), C.byref(top), C.byref(last)) == VDF_ERR_BAD_ARG
    assert call(13, 4, 13, 0, C.byref(r), C.byref(top), C.byref(last)) == VDF_ERR_BAD_ARG
    assert call(13, 4, 0, 0, None, C.byref(top), C.byref(last)) == VDF_ERR_BAD_ARG
