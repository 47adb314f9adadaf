"""GPU: the aggregate's device verifier with its per-entry Poseidon hashes made by vdf_ro_hash_batch
(vdf_nova_pp_set_verify_ro_device, include/vdf_nova.h).  The reference is the verifier the switch leaves alone: for every input
-- honest, damaged in the bytes, stated wrongly -- vdf_nova_verify_aggregate_device and vdf_nova_verify_aggregate_wire give the
same *ok, *bad_entry and decode code with the switch on as with it off, and both equal the host's vdf_nova_verify_aggregate
(test_gpu_aggregate_device.verdicts holds the three to each other).  vdf_nova_pp_verify_ro_stats tells which way a call went.
Every proof is made at t = 2."""
import os
import subprocess

import pytest

from test_gpu_aggregate_device import HEADER, Made, T, World, flipped, statement_bytes, verdicts
from test_gpu_lanes import host_lanes, lane_initials, traces_chain, zflat
from vdf_amd.minroot import PallasVDF, VestaVDF, State, FIELD_FP, FIELD_FQ
from vdf_amd.nova import (InverseMinRootCircuit, NovaVDFProof, RO_NEPTUNE_SHAPED, public_params, public_params_lanes, ro_preset,
                          verify_aggregate_wire)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 3, 5]
# offsets inside a statement of the wire: r_U1 (5 elements) | r_U2 (5) | l_u2 = comm_W, X[0], X[1] | T2 | z_i primary | z_i secondary
L_U2_W, L_U2_X0, L_U2_X1, T2_AT, ZI_AT = 320, 352, 384, 416, 448


@pytest.fixture(scope="module")
def world(ctx):
    pp = public_params(ctx, T)
    yield World(ctx, pp)
    pp.free()


def both_ways(ctx, made, data, stmt):
    """the three verifiers' common outcome with the switch off and with it on, held equal; the switch is left off"""
    pp = made.pp
    pp.set_verify_ro_device(0)
    off = verdicts(ctx, made, data, stmt)
    pp.set_verify_ro_device(1)
    try:
        assert pp.verify_ro_device == 1
        on = verdicts(ctx, made, data, stmt)
    finally:
        pp.set_verify_ro_device(0)
    assert on == off
    return on


def entries(K):
    return sorted({0, K // 2, K - 1})                     # the first, a middle and the last entry


def low_bit_flipped(element):
    raw = bytes(element)
    return bytes([raw[0] ^ 1]) + raw[1:]


def broken(made, what, e):
    """(data, stmt) with one break at entry e"""
    st = statement_bytes(made.arity)
    at = HEADER + e * st
    data = made.data
    steps, z0, zi = list(made.stmt[0]), [list(v) for v in made.stmt[1]], [list(v) for v in made.stmt[2]]
    if what == "zi: one bit":
        zi[e][1] = low_bit_flipped(zi[e][1])
    elif what == "zi on the wire: one bit":
        data = flipped(data, at + ZI_AT + 32)
    elif what == "num_steps":
        steps[e] += 1
    elif what == "z0":
        z0[e][0] = low_bit_flipped(z0[e][0])
    elif what == "l_u2.X[0]":
        data = flipped(data, at + L_U2_X0)
    elif what == "l_u2.X[1]":
        data = flipped(data, at + L_U2_X1)
    elif what == "T2":                                    # another point of the same curve: the entry's own l_u2.comm_W
        data = data[:at + T2_AT] + data[at + L_U2_W:at + L_U2_W + 32] + data[at + T2_AT + 32:]
        assert data != made.data
    else:
        raise KeyError(what)
    return data, (steps, z0, zi)


BREAKS = ("zi: one bit", "zi on the wire: one bit", "num_steps", "z0", "l_u2.X[0]", "l_u2.X[1]", "T2")


@pytest.mark.parametrize("K", KS)
def test_verdicts_do_not_depend_on_the_switch(ctx, world, K):
    made = world.aggregate(K)
    assert both_ways(ctx, made, made.data, made.stmt) == ("ok", (True, -1))
    for what in BREAKS:
        for e in entries(K):
            got = both_ways(ctx, made, *broken(made, what, e))
            if what == "T2":                              # another fold challenge: the accumulator is not the argument's
                assert got == ("ok", (False, -1)), (what, e)
            else:
                assert got == ("ok", (False, e)), (what, e)


@pytest.mark.parametrize("K", [3, 5])
def test_of_two_breaks_the_earlier_entry_is_named(ctx, world, K):
    made = world.aggregate(K)
    a, b = 0, K - 1
    for first, second in (("l_u2.X[0]", "zi: one bit"), ("zi: one bit", "l_u2.X[0]"), ("num_steps", "l_u2.X[1]"), ("l_u2.X[1]", "z0")):
        data, stmt = broken(made, first, a)
        once = Made.__new__(Made)
        once.pp, once.arity, once.data, once.stmt, once.K = made.pp, made.arity, data, stmt, K
        data2, stmt2 = broken(once, second, b)
        assert both_ways(ctx, made, data2, stmt2) == ("ok", (False, a)), (first, second)
        data, stmt = broken(made, first, b)               # ... and the other way round: the later kind at the earlier entry
        once.data, once.stmt = data, stmt
        data2, stmt2 = broken(once, second, a)
        assert both_ways(ctx, made, data2, stmt2) == ("ok", (False, a)), (second, first)


def test_stats_tell_which_way_a_call_went(ctx, world):
    pp = world.pp
    assert pp.verify_ro_device == 0                       # the default
    for K in KS:
        made = world.aggregate(K)
        before = pp.verify_ro_stats()
        assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
        assert verify_aggregate_wire(pp, made.data, *made.stmt) == (True, -1, 0)
        assert pp.verify_ro_stats() == before             # off: the host hashes
        pp.set_verify_ro_device(1)
        try:
            assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
            mid = pp.verify_ro_stats()
            assert (mid[0] - before[0], mid[1] - before[1]) == (3 * K, 3)
            assert verify_aggregate_wire(pp, made.data, *made.stmt) == (True, -1, 0)
            after = pp.verify_ro_stats()
            assert (after[0] - mid[0], after[1] - mid[1]) == (3 * K, 3)
            assert made.agg.verify(pp, *made.stmt) == (True, -1)                  # the host verifier does not read the switch
            assert pp.verify_ro_stats() == after
        finally:
            pp.set_verify_ro_device(0)
    pp.set_verify_ro_device(4)                            # from four entries on
    try:
        before = pp.verify_ro_stats()
        made = world.aggregate(3)
        assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
        assert pp.verify_ro_stats() == before
        made = world.aggregate(5)
        assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
        after = pp.verify_ro_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (15, 3)
    finally:
        pp.set_verify_ro_device(0)
    from vdf_amd.hip import VdfError
    with pytest.raises(VdfError) as e:
        pp.set_verify_ro_device(-1)
    assert e.value.code == 1 and pp.verify_ro_device == 0


def small_world(ctx, pp, items, arity=3):
    made = Made(pp, items, arity)
    assert both_ways(ctx, made, made.data, made.stmt) == ("ok", (True, -1))
    last = made.K - 1
    for what in ("zi: one bit", "num_steps", "l_u2.X[0]", "l_u2.X[1]"):
        assert both_ways(ctx, made, *broken(made, what, last)) == ("ok", (False, last)), what
    return made


def test_other_orientation(ctx):
    pp = public_params(ctx, T, field=FIELD_FP)
    items = []
    for x0, n in ((0x77, 1), (0x78, 2), (0x79, 1)):
        initial = State.from_ints(FIELD_FP, x0, 0, 0)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(VestaVDF.new(), T, n, initial)
        items.append((NovaVDFProof.prove_recursively(pp, circuits, T, z0), n, z0, [initial.x, initial.y, initial.i]))
    before = pp.verify_ro_stats()
    small_world(ctx, pp, items)
    assert pp.verify_ro_stats()[1] > before[1]
    pp.free()


def test_lanes_where_the_arity_is_above_three(ctx):
    L = 2
    pp = public_params_lanes(ctx, T, L)
    items = []
    for seed, n in ((61, 1), (62, 2)):
        inits, _ = lane_initials(L, seed)
        states, traces = host_lanes(T, n, inits)
        z0, lc = traces_chain(T, inits, traces)
        items.append((NovaVDFProof.prove_recursively(pp, lc, T, z0), n, z0, zflat(states[n])))
    before = pp.verify_ro_stats()
    small_world(ctx, pp, items, arity=3 * L)
    assert pp.verify_ro_stats()[1] > before[1]
    pp.free()


def test_another_ro_block_keeps_the_host_hashes(ctx):
    pp = public_params(ctx, T, ro=ro_preset(RO_NEPTUNE_SHAPED))
    items = []
    for x0, n in ((0x91, 1), (0x92, 2)):
        initial = State.from_ints(FIELD_FQ, x0, 0, 0)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), T, n, initial)
        items.append((NovaVDFProof.prove_recursively(pp, circuits, T, z0), n, z0, [initial.x, initial.y, initial.i]))
    small_world(ctx, pp, items)                           # the switch is accepted ...
    assert pp.verify_ro_stats() == (0, 0)                 # ... and the device oracle, family 0 only, is not used
    pp.free()


def test_the_c_verifier_takes_the_switch(world, tmp_path):
    exe = os.path.join(ROOT, "examples", "verify_aggregate")
    assert os.path.exists(exe), "examples/verify_aggregate is built by vdf_amd/csrc/Makefile (all)"
    made = world.aggregate(3)
    good, bad, stmt = tmp_path / "agg.bin", tmp_path / "bad.bin", tmp_path / "statements.txt"
    good.write_bytes(made.data)
    bad.write_bytes(flipped(made.data, HEADER + statement_bytes(3) + L_U2_X0))
    steps, z0, zi = made.stmt
    stmt.write_text("".join("%d %s %s\n" % (steps[k], " ".join(bytes(v).hex() for v in z0[k]), " ".join(bytes(v).hex() for v in zi[k]))
                            for k in range(3)))
    # fresh child processes (never an exec of this one: the test process has initialised the GPU), each under its own time limit
    for path, want in ((good, "count=3 ok=1 bad_entry=-1 decode_code=0"), (bad, "count=3 ok=0 bad_entry=1 decode_code=0")):
        for extra in ([], ["1"]):
            r = subprocess.run([exe, str(T), str(path), str(stmt)] + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert r.stdout.strip() == want, extra
