"""CPU: the Python wrappers of the aggregate's device verifier (vdf_amd/nova.py) refuse statements and byte strings of the wrong
shape themselves, before any library call -- the parameter set handed in here raises when its handle is asked for."""
import pytest

from vdf_amd import nova


class NoHandle:
    arity = 3

    @property
    def handle(self):
        raise AssertionError("the library was reached")


E = bytes(32)
INST = bytes(nova.WIRE_INSTANCE_BYTES)


@pytest.mark.parametrize("steps, z0, zi", [([1, 2], [[E] * 3], [[E] * 3] * 2),            # one z0 for two entries
                                           ([1], [[E] * 3], []),                           # no zi
                                           ([1], [[E] * 2], [[E] * 3]),                    # an entry of the wrong arity
                                           ([], [[E] * 3], [])])
def test_statements_of_the_wrong_shape(steps, z0, zi):
    with pytest.raises(ValueError):
        nova.verify_aggregate_wire(NoHandle(), b"VDFAGG01", steps, z0, zi)
    agg = nova.AggregateProof.__new__(nova.AggregateProof)
    agg.handle = None
    for device in (False, True):
        with pytest.raises(ValueError):
            agg.verify(NoHandle(), steps, z0, zi, device=device)


@pytest.mark.parametrize("instances, comm_TT", [([INST[:-1]], []), ([INST, INST], []), ([INST, INST], [E, E]), ([INST, INST], [E[:-1]]),
                                                ([INST], [E])])
def test_instances_of_the_wrong_shape(instances, comm_TT):
    with pytest.raises(ValueError):
        nova.aggregate_fold_instances_device(NoHandle(), 0, instances, comm_TT)
    with pytest.raises(ValueError):
        nova.aggregate_fold_instances(1, 0, E, instances, comm_TT)


def test_the_shapes_that_pass_reach_the_library():
    with pytest.raises(AssertionError, match="the library was reached"):
        nova.verify_aggregate_wire(NoHandle(), b"VDFAGG01", [1], [[E] * 3], [[E] * 3])
    with pytest.raises(AssertionError, match="the library was reached"):
        nova.aggregate_fold_instances_device(NoHandle(), 0, [INST, INST], [E])
