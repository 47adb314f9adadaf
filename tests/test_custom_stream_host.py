"""CPU tests of custom chains that grow (vdf_nova_custom_chain_begin, _push_checkpoints, _push_advice): the chain object is host-only
until materialize.  begin's refusals; a push that does not start on the chain's end names its lane and appends nothing; one hand-over
and one `every` per chain; a chain made whole does not grow; len and host_bytes; the rules of a table's rows."""
import functools

import numpy as np
import pytest

import forward_rebuild_spec as fs
import walks_spec
from rounds_spec import MOD, mont_rows
from vdf_amd._lib import VDF_ERR_BAD_ARG, VDF_ERR_BAD_LENGTH
from vdf_amd.hip import VdfError
from vdf_amd.nova import CHAIN_ASCENDING, CHAIN_DESCENDING, CustomChain, record_forward_body, record_walk_body, FIELD_FQ

T, EVERY, STEPS, ROWS, NA = 8, 4, 5, 4, 4
FIELD = FIELD_FQ
PER = T // EVERY


@functools.lru_cache(maxsize=None)
def forward_tape():
    return record_forward_body(fs.rescue_forward_body(FIELD, fs.rescue_table(FIELD, ROWS)[1]), FIELD)


@functools.lru_cache(maxsize=None)
def chains_of(lanes):
    starts = mont_rows([v for l in range(lanes) for v in (0x51DE + l, 3 * l, 0, 0)], MOD[FIELD])
    return fs.lane_chains(FIELD, forward_tape(), lanes, 0, None, starts, STEPS * T, [0] * lanes)


def initial(lanes):
    return np.concatenate([c[:NA] for c in chains_of(lanes)])


def step_checkpoints(lanes, g):
    return np.concatenate([c[g * T * NA:(g * T + T + 1) * NA].reshape(-1, 4 * NA)[::EVERY].reshape(-1, 4) for c in chains_of(lanes)])


def begin(lanes=1, direction=CHAIN_ASCENDING, **kw):
    return CustomChain.begin(FIELD, forward_tape(), direction, None, T, initial(lanes), lanes, **kw)


def refused(call, text, code=VDF_ERR_BAD_ARG):
    with pytest.raises(VdfError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_begin_refuses():
    tape, ini = forward_tape(), initial(1)
    refused(lambda: CustomChain.begin(FIELD, tape, 2, None, T, ini), "direction must be")
    refused(lambda: CustomChain.begin(7, tape, CHAIN_ASCENDING, None, T, ini), "unknown field")
    refused(lambda: CustomChain.begin(FIELD, tape, CHAIN_ASCENDING, None, 0, ini), "t out of range")
    refused(lambda: CustomChain.begin(FIELD, tape, CHAIN_ASCENDING, None, 2**31, ini), "t out of range")
    refused(lambda: CustomChain.begin(FIELD, tape, CHAIN_ASCENDING, None, T, ini, lanes=0), "lanes must be")
    refused(lambda: CustomChain.begin(FIELD, tape, CHAIN_ASCENDING, None, T, np.zeros((17 * NA, 4), dtype="<u8"), lanes=17), "lanes must be")
    # a forward tape with powers is no walk tape, and a walk tape no forward tape
    refused(lambda: CustomChain.begin(FIELD, tape, CHAIN_DESCENDING, None, T, ini), "")
    walk = record_walk_body(walks_spec.minroot_body(FIELD), FIELD)
    refused(lambda: CustomChain.begin(FIELD, walk, CHAIN_ASCENDING, mont_rows([0], MOD[FIELD]), T, ini[:2]), "")
    chain = CustomChain.begin(FIELD, walk, CHAIN_DESCENDING, mont_rows([7], MOD[FIELD]), T, ini[:2])
    assert chain.direction == CHAIN_DESCENDING and len(chain) == 0 and chain.n_adv == 2
    chain.free()


def test_the_rows_of_a_table_divide_t_and_every_j_base():
    tape = forward_tape()
    refused(lambda: CustomChain.begin(FIELD, tape, CHAIN_ASCENDING, None, 6, initial(1)), "tab_rows must divide t")
    refused(lambda: CustomChain.begin(FIELD, tape, CHAIN_ASCENDING, None, T, initial(3), lanes=3, j_base=[0, 8, 6]), "tab_rows must divide every j_base")
    chain = CustomChain.begin(FIELD, tape, CHAIN_ASCENDING, None, T, initial(3), lanes=3, j_base=[0, 8, 2**64 - 4])
    assert chain.lanes == 3 and len(chain) == 0
    chain.free()


@pytest.mark.parametrize("lanes", [1, 3])
def test_a_chain_grows_by_checkpoints(lanes):
    chain = begin(lanes)
    assert len(chain) == 0 and chain.direction == CHAIN_ASCENDING and chain.memory() == (0, 0)
    at_begin = chain.host_bytes()
    for g in range(STEPS):
        good = step_checkpoints(lanes, g)
        # the last lane does not start on the chain's end: named, and nothing is appended
        bad = good.copy()
        bad[(lanes - 1) * (PER + 1) * NA + 1, 0] ^= np.uint64(1)
        refused(lambda: chain.push_checkpoints(EVERY, bad), "lane %d: the step does not start on the chain's end" % (lanes - 1))
        if g:                                            # ... nor does the step before it, pushed again
            refused(lambda: chain.push_checkpoints(EVERY, step_checkpoints(lanes, g - 1)), "lane 0: the step does not start on the chain's end")
        assert len(chain) == g and chain.host_bytes() == at_begin + g * lanes * PER * NA * 32
        chain.push_checkpoints(EVERY, good)
        assert len(chain) == g + 1 and chain.every == EVERY
        # one hand-over, one `every`
        refused(lambda: chain.push_advice(np.zeros((lanes * (T + 1) * NA, 4), dtype="<u8")), "one hand-over per chain")
        refused(lambda: chain.push_checkpoints(2, np.zeros((lanes * 5 * NA, 4), dtype="<u8")), "the chain's first push said 4")
        refused(lambda: chain.push_checkpoints(3, good), "must be positive and divide t")
        refused(lambda: chain.push_checkpoints(0, good), "must be positive and divide t")
        assert len(chain) == g + 1
    assert chain.host_bytes() == at_begin + STEPS * lanes * PER * NA * 32
    if lanes > 1:
        refused(lambda: chain.push_checkpoints(EVERY, step_checkpoints(lanes, 0), lane_stride=PER), "lane_stride must be at least")
    # released steps keep their checkpoints; a range beyond the chain is refused
    chain.release(0, STEPS)
    assert chain.host_bytes() == at_begin + STEPS * lanes * PER * NA * 32 and chain.memory() == (0, 0)
    refused(lambda: chain.release(STEPS, 1), "step range out of bounds", VDF_ERR_BAD_LENGTH)
    chain.free()


@pytest.mark.parametrize("lanes", [1, 3])
def test_a_chain_grows_by_whole_traces(lanes):
    chain = begin(lanes)
    at_begin, step_bytes = chain.host_bytes(), lanes * (T + 1) * NA * 32
    for g in range(STEPS):
        good = fs.step_advice(chains_of(lanes), NA, T, g)
        bad = good.copy()
        bad[(lanes - 1) * (T + 1) * NA + 3, 2] ^= np.uint64(1)
        refused(lambda: chain.push_advice(bad), "lane %d: the step does not start on the chain's end" % (lanes - 1))
        assert len(chain) == g
        # lanes two entries further apart than they need be
        wide = np.zeros(((lanes - 1) * (T + 3) + T + 1, NA * 4), dtype="<u8")
        for l in range(lanes):
            wide[l * (T + 3):l * (T + 3) + T + 1] = good.reshape(lanes, T + 1, NA * 4)[l]
        chain.push_advice(wide.reshape(-1, 4), lane_stride=T + 3)
        assert len(chain) == g + 1 and chain.host_bytes() == at_begin + (g + 1) * step_bytes
        refused(lambda: chain.push_checkpoints(EVERY, step_checkpoints(lanes, g)), "one hand-over per chain")
    if lanes > 1:
        refused(lambda: chain.push_advice(np.zeros((lanes * (T + 1) * NA, 4), dtype="<u8"), lane_stride=T), "lane_stride must be at least")
    # the host copy of a released step goes
    chain.release(1, 3)
    assert chain.host_bytes() == at_begin + 2 * step_bytes
    chain.release(0, STEPS)
    assert chain.host_bytes() == at_begin and len(chain) == STEPS
    chain.free()


def test_a_chain_made_whole_does_not_grow():
    cps = np.concatenate([c.reshape(-1, 4 * NA)[::EVERY].reshape(-1, 4) for c in chains_of(1)])
    chain = CustomChain.from_checkpoints(FIELD, forward_tape(), None, T, EVERY, STEPS, cps, forward=True)
    before = chain.host_bytes()
    refused(lambda: chain.push_checkpoints(EVERY, step_checkpoints(1, 0)), "only a chain of vdf_nova_custom_chain_begin grows")
    refused(lambda: chain.push_advice(fs.step_advice(chains_of(1), NA, T, 0)), "only a chain of vdf_nova_custom_chain_begin grows")
    assert len(chain) == STEPS and chain.host_bytes() == before
    chain.free()
