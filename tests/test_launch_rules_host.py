"""CPU: every row of launch_rules_spec through the host restatements of libvdf_nova.so (include/vdf_nova.h vdf_nova_*_eval), which
read what a launch is refused for from the headers the launchers read (vdf_amd/csrc/tape_launch.h, periodic_rules.h).  A refused
call answers with the row's code and words and writes nothing; the valid call made after it gives the bytes it gave before; and a
call that breaks two consecutive rules is answered by the earlier one.  (The same table against the launchers, and the two
libraries' answers against each other: test_gpu_launch_rules.py.)"""
import functools

import pytest

import launch_rules_spec as spec
from vdf_amd.nova import nova_lib


def evaluate(entry, call):
    """(code, message) of the restatement"""
    rc = getattr(nova_lib, spec.FUNCTIONS[entry][0])(*spec.host_args(entry, call))
    return rc, (nova_lib.vdf_nova_last_error() or b"").decode() if rc else ""


@functools.lru_cache(maxsize=None)
def valid_bytes(entry):
    """what the valid call leaves in its arrays, made once"""
    call = spec.valid_call(entry)
    assert evaluate(entry, call) == (spec.VDF_OK, "")
    after = spec.snapshot(call)
    assert after != spec.snapshot(spec.valid_call(entry))      # (it ran)
    return after


def answer(entry, mutations, code, pattern):
    before = valid_bytes(entry)
    call = spec.valid_call(entry)
    try:
        for mutate in mutations:
            mutate(call)
        held = spec.snapshot(call)
        got = evaluate(entry, call)
    finally:
        spec.undo(call)
    print(entry, got)
    assert got[0] == code and pattern in got[1]
    if code != spec.VDF_OK or not call.get("n", 1) or not call.get("rounds", 1) or not call.get("reps", 1):
        assert spec.snapshot(call) == held             # refused, or nothing to do: nothing is written
    again = spec.valid_call(entry)
    assert evaluate(entry, again) == (spec.VDF_OK, "") and spec.snapshot(again) == before


@pytest.mark.parametrize("row", spec.rows(), ids=spec.row_id)
def test_a_row_is_answered_as_the_table_says_and_writes_nothing(row):
    answer(row.entry, [row.mutate], row.code, row.pattern)


@pytest.mark.parametrize("pair", spec.pairs(), ids=lambda p: spec.row_id(p[0]) + "+" + spec.row_id(p[1]))
def test_of_two_consecutive_rules_the_earlier_one_is_named(pair):
    first, second = pair
    assert first.entry == second.entry and first.rule < second.rule
    answer(first.entry, [second.mutate, first.mutate], first.code, first.pattern)


def test_the_table_has_a_row_for_every_rule_of_every_entry_point():
    rules = {e: sorted({r.rule for r in spec.rows() if r.entry == e}) for e in spec.ENTRIES}
    assert rules["run"] == [1, 2, 5] and rules["run_lanes"] == [1, 2, 3, 4, 5, 6]
    assert rules["walk"] == [1, 4, 6, 7, 8, 9, 10, 11, 12, 13] and rules["walk_lanes"] == list(range(1, 14))
    assert rules["forward_walk"] == [1, 4, 6, 7, 8, 9, 10, 11] and rules["rebuild_lanes"] == list(range(1, 13))
    assert rules["periodic"] == list(range(1, 12))
