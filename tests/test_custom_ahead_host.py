"""CPU: the host side of a custom chain's lookahead and early rows (include/vdf_nova.h tuning.custom_ahead).

a. the tuning field: 0 by default, 0 for a caller whose struct is the one of before the field, refused outside 0 .. 2, and its
   environment override;
b. vdf_nova_shape_early_rows_custom against a numpy model of the rule over the triples of shape_export_custom: FC's run is exactly
   the repeat's rows in both fields, with z_in where the triples say it is; t = 5 is under the floor of 64 rows; a variable between
   z_in and the repeat moves the segment and nothing else; an inv that is a variable of the circuit's own leaves no early rows;
c. the built-in kinds' early rows are the ones of before the rule was generalised (literals recorded from that build)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from custom_ahead_spec import FC, FCgap, FCown, cols_of_row, early_run_model
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.nova import (CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_FORWARD, CIRCUIT_MINROOT_REFERENCE, FIELD_FP, FIELD_FQ, NovaTuning,
                          shape_early_rows_custom, shape_export_custom, shape_periodic_custom, shape_stencil, shape_stencil_field,
                          shape_stencil_lanes, tuning_default, tuning_read)

T = 65


# ---- a. the tuning field ---------------------------------------------------------------------------------------------------------
def test_the_default_is_todays_schedule():
    assert tuning_default().custom_ahead == 0
    assert tuning_read(None).custom_ahead == 0
    assert NovaTuning._fields_[-1][0] == "custom_ahead"                     # at the end of the struct


def test_a_struct_of_before_the_field_reads_as_zero():
    t = tuning_default(custom_ahead=2, periodic_rows=1)
    assert tuning_read(t).custom_ahead == 2
    old = NovaTuning.custom_ahead.offset                                    # sizeof(vdf_nova_tuning) of a caller without the field
    got = tuning_read(t, struct_size=old)
    assert got.custom_ahead == 0 and got.periodic_rows == 1 and got.struct_size == C.sizeof(NovaTuning)
    for size in (old - 4, old + 1, C.sizeof(NovaTuning) + 8, 0):
        with pytest.raises(VdfError) as e:
            tuning_read(t, struct_size=size)
        assert e.value.code == VDF_ERR_BAD_ARG


@pytest.mark.parametrize("bad", [3, -1])
def test_a_value_outside_0_to_2_is_refused(bad):
    with pytest.raises(VdfError) as e:
        tuning_read(tuning_default(custom_ahead=bad))
    assert e.value.code == VDF_ERR_BAD_ARG
    for good in (0, 1, 2):
        assert tuning_read(tuning_default(custom_ahead=good)).custom_ahead == good


@pytest.mark.parametrize("value,want", [("2", 2), ("7", 0)])
def test_the_environment_override(value, want):
    """VDF_NOVA_CUSTOM_AHEAD is read once per process, by the first vdf_nova_tuning_default: a child process; out of range = ignored"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "from vdf_amd.nova import tuning_default; print(tuning_default().custom_ahead)"],
                       cwd=root, env=dict(os.environ, VDF_NOVA_CUSTOM_AHEAD=value), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == str(want), r.stdout + r.stderr


# ---- b. which rows are early -----------------------------------------------------------------------------------------------------
def shape_facts(circuit, field):
    """(triples, num_cons, num_vars, first variable of the repeat, first row of the repeat) from the host-only exports"""
    mats = shape_export_custom(circuit, field, 0)
    pr, info = shape_periodic_custom(circuit, field)
    assert pr is not None
    return mats, info["num_cons"], info["num_cols"] - 3, info["seg_begin"], pr.row_begin - pr.lead * 3


def zin_from_triples(mats, row0, seg):
    """where z_in is, read off the repeat's own rows: repetition 0 enforces t2 * xn = x + y over z_in's x and y, and repetition 1's
    y is x + i_in + 0"""
    zx, zy = cols_of_row(mats[2], row0 + 2)
    first, zi = [c for c in cols_of_row(mats[2], row0 + 5) if c < seg]       # (the third entry is repetition 0's root, in the segment)
    assert (first, zy, zi) == (zx, zx + 1, zx + 2)
    return zx


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_fcs_early_rows_are_exactly_the_repeats_rows(field):
    c = FC(T, field)
    mats, num_cons, num_vars, seg, row0 = shape_facts(c, field)
    got = shape_early_rows_custom(c, field)
    zin = zin_from_triples(mats, row0, seg)
    assert got == dict(row_begin=row0, rows=3 * T, zin_begin=zin, seg_begin=seg)
    assert zin + 3 == seg                                                   # FC allocates nothing of its own in front of the repeat
    assert (got["row_begin"], got["rows"]) == early_run_model(mats, num_cons, num_vars, seg, 3 * T, zin, 3)


def test_fifteen_rows_are_under_the_floor():
    c = FC(5)
    mats, num_cons, num_vars, seg, row0 = shape_facts(c, FIELD_FQ)
    got = shape_early_rows_custom(c)
    assert (got["row_begin"], got["rows"]) == (0, 0) and got["seg_begin"] == seg and got["zin_begin"] == zin_from_triples(mats, row0, seg)
    assert early_run_model(mats, num_cons, num_vars, seg, 15, got["zin_begin"], 3) == (0, 0)
    assert early_run_model(mats, num_cons, num_vars, seg, 15, got["zin_begin"], 3, floor=1) == (row0, 15)      # the run is there, only short


def test_a_variable_between_z_in_and_the_repeat_moves_the_segment_only():
    plain, gap = shape_early_rows_custom(FC(T)), shape_early_rows_custom(FCgap(T))
    assert gap == dict(plain, seg_begin=plain["seg_begin"] + 1)
    c = FCgap(T)
    mats, num_cons, num_vars, seg, row0 = shape_facts(c, FIELD_FQ)
    assert gap["zin_begin"] == zin_from_triples(mats, row0, seg) and gap["zin_begin"] + 4 == seg
    assert (gap["row_begin"], gap["rows"]) == early_run_model(mats, num_cons, num_vars, seg, 3 * T, gap["zin_begin"], 3) == (row0, 3 * T)
    # the rule of before -- z_in taken to sit right in front of the segment -- would have lost the rows that read z_in.x
    assert early_run_model(mats, num_cons, num_vars, seg, 3 * T, seg - 3, 3)[1] < 3 * T


def test_an_inv_of_the_circuits_own_leaves_no_early_rows():
    c = FCown(T)
    mats, num_cons, num_vars, seg, row0 = shape_facts(c, FIELD_FQ)
    got = shape_early_rows_custom(c)
    assert (got["row_begin"], got["rows"]) == (0, 0)
    # every third row reads the circuit's own variable: no run of 64
    assert early_run_model(mats, num_cons, num_vars, seg, 3 * T, got["zin_begin"], 3) == (0, 0)
    assert got["zin_begin"] + 4 == seg


# ---- c. the built-in kinds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,code", [(CIRCUIT_MINROOT_BOUND, 3), (CIRCUIT_MINROOT_REFERENCE, 4), (CIRCUIT_MINROOT_FORWARD, 5)])
def test_the_built_in_kinds_keep_their_early_rows(kind, code):
    """(stencil code, first early row, early rows, first round variable) as the build before this rule gave them"""
    assert shape_stencil(24, kind) == (code, 8605, 73, 8613)
    assert shape_stencil(65, kind) == (code, 8605, 196, 8613)
    assert shape_stencil_field(FIELD_FP, 65, kind) == (code, 8605, 196, 8613)
    if kind == CIRCUIT_MINROOT_FORWARD:
        assert shape_stencil_lanes(24, 3) == (6, 9667, 219, 9687)
