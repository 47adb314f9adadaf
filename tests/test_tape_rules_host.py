"""CPU: the rules of a round tape, stated once in vdf_amd/csrc/tape_rules.h, as the host evaluators of all three modes apply them
(vdf_nova_round_tape_eval, vdf_nova_walk_tape_eval, vdf_nova_forward_tape_eval): every tape of tape_rules_spec.cases() is refused
with VDF_ERR_BAD_ARG, the message names the op or the variable, and nothing is written; the valid tape of each mode runs.
tests/test_gpu_tape_interpreter.py sends the same table through libvdf_hip.so's launchers."""
import ctypes as C
import re

import numpy as np
import pytest

from rounds_spec import MOD, mont_rows
from tape_rules_spec import FORWARD, MODES, N_ADV, ROUND, SENTINEL, WALK, base_tape, cases
from vdf_amd._lib import VDF_ERR_BAD_ARG, VDF_OK
from vdf_amd.minroot import nova_lib
from vdf_amd.nova import FIELD_FP, FIELD_FQ


def sentinel(n_elems):
    return np.full((n_elems, 4), SENTINEL, dtype="<u8")


def host_run(mode, field, tape):
    """one repetition / one walk of one round through the host entry point of `mode`: (status, message, the arrays the call may
    write, as they were before the call, the same after it)"""
    m = MOD[field]
    inv = mont_rows([3], m)
    tp = C.addressof(tape.c)
    if mode == ROUND:
        advice, out = mont_rows([5, 6, 8, 9], m), sentinel(N_ADV)
        bufs = [out]
        before = [b.copy() for b in bufs]
        rc = nova_lib.vdf_nova_round_tape_eval(field, tp, 1, inv.ctypes.data, advice.ctypes.data, out.ctypes.data)
    elif mode == WALK:
        entries, trace = mont_rows([5, 6], m), sentinel(2 * N_ADV)
        bufs = [entries, trace]
        before = [b.copy() for b in bufs]
        rc = nova_lib.vdf_nova_walk_tape_eval(field, tp, inv.ctypes.data, entries.ctypes.data, 1, 1, trace.ctypes.data, 0, 1, 0, 0, 7, 0, 1, None, None)
    else:
        entries, cps, trace = mont_rows([5, 6], m), sentinel(2 * N_ADV), sentinel(2 * N_ADV)
        bufs = [entries, cps, trace]
        before = [b.copy() for b in bufs]
        rc = nova_lib.vdf_nova_forward_tape_eval(field, tp, inv.ctypes.data, entries.ctypes.data, 1, 1, cps.ctypes.data, 1, 2, trace.ctypes.data, 2, 0,
                                                 7, 0)
    return rc, (nova_lib.vdf_nova_last_error() or b"").decode(), before, bufs


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("mode", MODES)
def test_the_valid_tape_of_each_mode_runs(mode, field):
    rc, msg, before, after = host_run(mode, field, base_tape(mode, field))
    assert rc == VDF_OK, msg
    for b, a in zip(before, after):                    # the variables, the landing, the trace and the checkpoint were written
        assert (a != b).any()
    if mode == ROUND:
        assert not (after[0] == np.uint64(SENTINEL)).any()


def test_a_forward_tape_is_no_round_tape_and_no_descending_tape():
    """the tape with every op is valid in one mode only: its POW, its POWC and (descending) its ADV are refused elsewhere"""
    for mode in (ROUND, WALK):
        rc, msg, before, after = host_run(mode, FIELD_FQ, base_tape(FORWARD, FIELD_FQ))
        assert rc == VDF_ERR_BAD_ARG and "malformed" in msg, msg
        assert all(np.array_equal(b, a) for b, a in zip(before, after))


@pytest.mark.parametrize("name,modes,mutate,names", cases(), ids=[c[0] for c in cases()])
def test_every_broken_rule_is_refused_in_every_mode_and_nothing_is_written(name, modes, mutate, names):
    for mode in modes:
        tape = base_tape(mode, FIELD_FQ)
        mutate(tape)
        rc, msg, before, after = host_run(mode, FIELD_FQ, tape)
        assert rc == VDF_ERR_BAD_ARG, (mode, rc, msg)
        assert re.search(names, msg), (mode, msg)
        assert all(np.array_equal(b, a) for b, a in zip(before, after)), mode
