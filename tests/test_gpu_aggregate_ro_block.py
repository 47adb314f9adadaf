"""GPU: the aggregate's device verifier under ANOTHER random-oracle block (family 1) with its per-entry Poseidon hashes made by
vdf_ro_hash_batch_block (vdf_nova_pp_set_verify_ro_block_device, include/vdf_nova.h).  The reference is the verifier the switch
leaves alone: for every input -- honest, damaged in the bytes, stated wrongly -- vdf_nova_verify_aggregate_device and
vdf_nova_verify_aggregate_wire give the same *ok, *bad_entry and decode code with the new switch on as with it off, and both
equal the host's vdf_nova_verify_aggregate (test_gpu_aggregate_device.verdicts holds the three to each other).
vdf_nova_pp_verify_ro_stats tells which way a call went.  Two blocks: the neptune-shaped one (width 25, 8 + 57 rounds) and a
small one (width 9, 8 + 30).  Every proof is made at t = 2; three proofs per set, named cyclically."""
import pytest

from test_gpu_aggregate_device import Made, T, verdicts
from test_gpu_aggregate_ro import broken
from vdf_amd.hip import VdfError
from vdf_amd.minroot import PallasVDF, State, FIELD_FQ
from vdf_amd.nova import InverseMinRootCircuit, NovaVDFProof, RO_NEPTUNE_SHAPED, public_params, ro_preset, verify_aggregate_wire

pytestmark = pytest.mark.gpu
KS = [1, 2, 3, 5]
BLOCKS = {"neptune-shaped": {}, "width 9": {"width": 9, "partial_rounds": 30}}


class BlockWorld:
    """three distinct proofs (1, 2 and 1 steps) under one parameter set made under `ro`, and the aggregates that name them cyclically"""
    def __init__(self, ctx, ro):
        self.pp = public_params(ctx, T, ro=ro)
        self.items = []
        for x0, n in ((0x91, 1), (0x92, 2), (0x93, 1)):
            initial = State.from_ints(FIELD_FQ, x0, 0, 0)
            z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), T, n, initial)
            self.items.append((NovaVDFProof.prove_recursively(self.pp, circuits, T, z0), n, z0, [initial.x, initial.y, initial.i]))
        self.made = {}

    def aggregate(self, K):
        if K not in self.made:
            self.made[K] = Made(self.pp, [self.items[k % len(self.items)] for k in range(K)])
        return self.made[K]


@pytest.fixture(scope="module", params=list(BLOCKS))
def world(ctx, request):
    w = BlockWorld(ctx, ro_preset(RO_NEPTUNE_SHAPED, **BLOCKS[request.param]))
    yield w
    w.pp.free()


@pytest.fixture(scope="module")
def default_world(ctx):
    w = BlockWorld(ctx, None)
    yield w
    w.pp.free()


def both_ways(ctx, made, data, stmt):
    """the three verifiers' common outcome with the new switch off and with it on, held equal; the switch is left off"""
    pp = made.pp
    pp.set_verify_ro_block_device(0)
    off = verdicts(ctx, made, data, stmt)
    pp.set_verify_ro_block_device(1)
    try:
        assert pp.verify_ro_block_device == 1
        on = verdicts(ctx, made, data, stmt)
    finally:
        pp.set_verify_ro_block_device(0)
    assert on == off
    return on


@pytest.mark.parametrize("K", KS)
def test_verdicts_do_not_depend_on_the_switch(ctx, world, K):
    made = world.aggregate(K)
    before = world.pp.verify_ro_stats()
    assert both_ways(ctx, made, made.data, made.stmt) == ("ok", (True, -1))
    after = world.pp.verify_ro_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (6 * K, 6)          # the device call and the wire call, the switch on
    for what in ("zi: one bit", "num_steps", "l_u2.X[0]", "l_u2.X[1]"):
        for e in sorted({0, K - 1}):                                              # the first and the last entry
            assert both_ways(ctx, made, *broken(made, what, e)) == ("ok", (False, e)), (what, e)


def test_of_two_breaks_the_earlier_entry_is_named(ctx, world):
    made = world.aggregate(5)
    data, stmt = broken(made, "l_u2.X[1]", 1)
    once = Made.__new__(Made)
    once.pp, once.arity, once.data, once.stmt, once.K = made.pp, made.arity, data, stmt, 5
    assert both_ways(ctx, made, *broken(once, "zi: one bit", 4)) == ("ok", (False, 1))
    assert both_ways(ctx, made, *broken(once, "num_steps", 0)) == ("ok", (False, 0))


def test_stats_tell_which_way_a_call_went(ctx, world):
    pp = world.pp
    assert pp.verify_ro_block_device == 0                                         # the default
    for K in KS:
        made = world.aggregate(K)
        before = pp.verify_ro_stats()
        assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
        assert verify_aggregate_wire(pp, made.data, *made.stmt) == (True, -1, 0)
        assert pp.verify_ro_stats() == before                                     # off: the host hashes
        pp.set_verify_ro_device(1)                                                # the OLD switch alone: accepted, the host hashes
        try:
            assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
            assert verify_aggregate_wire(pp, made.data, *made.stmt) == (True, -1, 0)
            assert pp.verify_ro_stats() == before
        finally:
            pp.set_verify_ro_device(0)
        pp.set_verify_ro_block_device(1)
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
            pp.set_verify_ro_block_device(0)
    pp.set_verify_ro_block_device(4)                                              # from four entries on
    try:
        assert pp.verify_ro_block_device == 4
        before = pp.verify_ro_stats()
        made = world.aggregate(3)
        assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
        assert pp.verify_ro_stats() == before
        made = world.aggregate(5)
        assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
        after = pp.verify_ro_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (15, 3)
    finally:
        pp.set_verify_ro_block_device(0)


def test_a_negative_value_is_refused(world):
    pp = world.pp
    with pytest.raises(VdfError) as e:
        pp.set_verify_ro_block_device(-1)
    assert e.value.code == 1 and pp.verify_ro_block_device == 0
    assert pp.verify_ro_device == 0                                               # the two switches are two values
    pp.set_verify_ro_block_device(7)
    assert (pp.verify_ro_block_device, pp.verify_ro_device) == (7, 0)
    pp.set_verify_ro_block_device(0)


def test_a_default_block_set_ignores_the_new_switch(ctx, default_world):
    pp = default_world.pp
    made = default_world.aggregate(3)
    pp.set_verify_ro_block_device(1)                                              # accepted ...
    try:
        assert pp.verify_ro_block_device == 1
        before = pp.verify_ro_stats()
        assert verdicts(ctx, made, made.data, made.stmt) == ("ok", (True, -1))
        assert pp.verify_ro_stats() == before                                     # ... and not read: the host hashes
        pp.set_verify_ro_device(1)                                                # its stats move under the old switch alone
        assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
        after = pp.verify_ro_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (9, 3)
        pp.set_verify_ro_block_device(0)
        assert made.agg.verify(pp, *made.stmt, device=True) == (True, -1)
        assert tuple(a - b for a, b in zip(pp.verify_ro_stats(), after)) == (9, 3)
    finally:
        pp.set_verify_ro_device(0)
        pp.set_verify_ro_block_device(0)
