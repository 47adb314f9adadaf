"""GPU: every row of launch_rules_spec through the launcher of libvdf_hip.so and through the restatement of libvdf_nova.so in the
same process, each with its pointers where it wants them (the launcher's vectors in device memory; the tape, inv, j_base and u1 on
the host): the two answers are equal in code and in the whole text of the message, a refused launch writes nothing, a call that
breaks two consecutive rules is answered by the earlier one on both sides, and the valid call leaves the same bytes on both.  No
row launches more than 3 walks of 2 rounds; a refusal launches nothing."""

import numpy as np
import pytest

import launch_rules_spec as spec
from test_launch_rules_host import evaluate
from vdf_amd._lib import lib

pytestmark = pytest.mark.gpu


def launch(ctx, entry, call):
    """(code, message, the bytes of the call's arrays afterwards) of the launcher"""
    import torch
    on_device = {}

    def place(name, array):
        if name in spec.HOST_ARRAYS:
            return array.ctypes.data
        on_device[name] = torch.from_numpy(array.view(np.uint8).reshape(-1)).cuda()
        return on_device[name].data_ptr()
    rc = getattr(lib, spec.FUNCTIONS[entry][1])(ctx.handle, *spec.host_args(entry, call, place))
    msg = (lib.vdf_last_error(ctx.handle) or b"").decode() if rc else ""
    ctx.sync()
    after = spec.snapshot(call)
    after.update({name: t.cpu().numpy().tobytes() for name, t in on_device.items()})
    return rc, msg, after


def both(ctx, entry, mutations):
    call = spec.valid_call(entry)
    try:
        for mutate in mutations:
            mutate(call)
        held = spec.snapshot(call)
        host = evaluate(entry, spec_copy(call))
        code, msg, after = launch(ctx, entry, call)
    finally:
        spec.undo(call)
    print(entry, (code, msg), host)
    return (code, msg), host, held, after, call


def spec_copy(call):
    """the call over copies of its arrays: the restatement works in place, and the launcher is to start from the same bytes"""
    return {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in call.items()}


def ran_nothing(call):
    return not call.get("n", 1) or not call.get("rounds", 1) or not call.get("reps", 1)


@pytest.mark.parametrize("entry", spec.ENTRIES)
def test_the_valid_call_leaves_the_restatements_bytes(ctx, entry):
    call = spec.valid_call(entry)
    on_host = spec_copy(call)
    assert evaluate(entry, on_host) == (spec.VDF_OK, "")
    code, msg, after = launch(ctx, entry, call)
    assert (code, msg) == (spec.VDF_OK, "")
    assert after == spec.snapshot(on_host) and after != spec.snapshot(call)


@pytest.mark.parametrize("row", spec.rows(), ids=spec.row_id)
def test_both_libraries_give_a_row_the_same_answer(ctx, row):
    got, host, held, after, call = both(ctx, row.entry, [row.mutate])
    assert host[0] == row.code and row.pattern in host[1]
    if row.launcher_reaches:
        assert got == host
    else:                                                  # a null vector: the launcher's own check of where the vectors live
        assert got[0] == spec.VDF_ERR_BAD_ARG and "live in device memory" in got[1]
    if got[0] != spec.VDF_OK or ran_nothing(call):
        assert after == held


@pytest.mark.parametrize("pair", spec.pairs(launcher=True), ids=lambda p: spec.row_id(p[0]) + "+" + spec.row_id(p[1]))
def test_both_libraries_name_the_earlier_of_two_broken_rules(ctx, pair):
    first, second = pair
    got, host, held, after, call = both(ctx, first.entry, [second.mutate, first.mutate])
    assert got == host and got[0] == first.code and first.pattern in got[1]
    if got[0] != spec.VDF_OK or ran_nothing(call):
        assert after == held
