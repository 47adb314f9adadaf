"""GPU: a custom chain's lookahead and early rows on the built-in schedule (include/vdf_nova.h tuning.custom_ahead: 1 = the next
step's rounds and their commitment on the lookahead queue, 2 = that and the early rows of T).

a. the running proof and the compressed proof are byte for byte those of the vdf_nova_prove_step_custom loop over host advice under
   the default tuning: every window length, the other orientation, periodic rows, a repeat under the floor of 64 rows, three lanes;
b. a value outside 0 .. 2 is refused;
c. it really ran ahead: the counts of vdf_nova_proof_ahead_stats;
d. a miss by another chain object, and a miss by an `inv` the probe did not see: the same bytes;
e. step-by-step driving over pending walks;
f. errors keep their names; g. plain vdf_nova_prove_step_custom is left alone."""
import functools

import numpy as np
import pytest

from custom_ahead_spec import FC, FCliar
from custom_chain_spec import FW, I0, X0, checkpoints_of, minroot_chain, step_traces, z0_of, zi_of
from custom_lanes_spec import FL, lanes_checkpoints, step_advice_ints, walk_inv_and_j_base, z_of
from rounds_spec import MOD, mont_rows
from walks_spec import minroot_body
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.nova import CustomChain, NovaVDFProof, public_params_custom, record_walk_body, FIELD_FP, FIELD_FQ

pytestmark = pytest.mark.gpu
T, EVERY, STEPS = 65, 13, 7
LANES, LANE_STEPS = 3, 3
_PP = {}


@pytest.fixture(scope="module", autouse=True)
def free_the_parameter_sets():
    yield
    for pp in _PP.values():
        pp.free()
    _PP.clear()
    reference.cache_clear()
    lanes_reference.cache_clear()


def params(ctx, mode, field=FIELD_FQ, t=T, periodic=0, cls=FC):
    """one parameter set per shape and tuning for the whole module"""
    key = (mode, field, t, periodic, cls.__name__)
    if key not in _PP:
        _PP[key] = public_params_custom(ctx, cls(t, field), field=field, periodic_rows=periodic, custom_ahead=mode)
    return _PP[key]


def chain_of(field=FIELD_FQ, t=T, every=EVERY, steps=STEPS, cps=None):
    m = MOD[field]
    good = checkpoints_of(minroot_chain(field, t, steps, X0, I0), 2, every, m)
    return CustomChain.from_checkpoints(field, record_walk_body(minroot_body(field), field), mont_rows([I0], m), t, every, steps,
                                        good if cps is None else cps)


def proof_bytes(pp, proof):
    snark = proof.compress(pp)
    out = proof.serialize(), snark.serialize()
    snark.free(); proof.free()
    return out


@functools.lru_cache(maxsize=None)
def reference(ctx, field=FIELD_FQ, t=T, cls=FC):
    """(running proof bytes, compressed proof bytes) of the plain loop under the DEFAULT tuning: vdf_nova_prove_step_custom step by
    step over HOST advice"""
    pp, c, proof = params(ctx, 0, field, t, 0, cls), cls(t, field), None
    for tr in step_traces(field, t, STEPS):
        c.advice = tr
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0_of(field))
    assert proof.verify(pp, STEPS, z0_of(field), zi_of(field, t, STEPS)) is True
    assert proof.ahead_stats() == (0, 0, 0)
    return proof_bytes(pp, proof)


def recursively(ctx, mode, window_steps, field=FIELD_FQ, t=T, every=EVERY, periodic=0, cls=FC, check_steps=False):
    """prove_recursively_custom under custom_ahead = mode: (proof bytes, ahead_stats)"""
    pp, chain = params(ctx, mode, field, t, periodic, cls), chain_of(field, t, every)
    proof = NovaVDFProof.prove_recursively_custom(pp, cls(t, field), chain, z0_of(field), window_steps=window_steps, check_steps=check_steps)
    assert proof.num_steps() == STEPS and chain.memory() == (0, 0)
    stats = proof.ahead_stats()
    chain.free()
    return proof_bytes(pp, proof), stats


# ---- a. the same bytes, c. it really ran ahead ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("window_steps", [2, 3, 100])
def test_the_proof_is_the_plain_loops_and_the_lookahead_ran(ctx, mode, window_steps):
    pp = params(ctx, mode)
    rb, n_cons, t = pp.repeat_rows()
    assert pp.early_rows() == ((rb, n_cons * t) if mode == 2 else (0, 0)) and pp.stencil() == 0
    got, (hits, misses, skipped) = recursively(ctx, mode, window_steps)
    assert got == reference(ctx)
    if window_steps == 100:                            # the whole chain in window 0, waited for
        assert (hits, misses, skipped) == (STEPS - 1, 0, 0)
    else:                                              # a window's first step comes before its walks are resolved
        assert hits + skipped == STEPS - 1 and misses == 0 and hits >= 1


def test_default_tuning_counts_nothing(ctx):
    got, stats = recursively(ctx, 0, 3)
    assert got == reference(ctx) and stats == (0, 0, 0)
    assert params(ctx, 0).early_rows() == (0, 0) and params(ctx, 0).tuning()["custom_ahead"] == 0


def test_the_other_orientation(ctx):
    got, stats = recursively(ctx, 2, 3, field=FIELD_FP)
    assert got == reference(ctx, FIELD_FP) and stats[1] == 0 and stats[0] >= 1


def test_periodic_rows_on_the_early_rows_queue(ctx):
    pp = params(ctx, 2, periodic=1)
    rb, n_cons, t = pp.repeat_rows()
    assert pp.stencil() == 7 and pp.early_rows() == (rb, n_cons * t) and pp.periodic_rows() is not None
    got, stats = recursively(ctx, 2, 100, periodic=1, check_steps=True)      # (every step's fresh instance scanned: its own A z, B z, C z are
    assert got == reference(ctx) and stats == (STEPS - 1, 0, 0)              # overwritten by the next step's early rows, and made again)


def test_a_repeat_under_the_floor_has_no_early_rows(ctx):
    pp = params(ctx, 2, t=5)
    assert pp.early_rows() == (0, 0)
    got, stats = recursively(ctx, 2, 100, t=5, every=5)
    assert got == reference(ctx, t=5) and stats == (STEPS - 1, 0, 0)


@functools.lru_cache(maxsize=None)
def lanes_reference(ctx):
    field, m = FIELD_FQ, MOD[FIELD_FQ]
    key = (0, "lanes")
    _PP[key] = public_params_custom(ctx, FL(T, LANES, "repeat", field), field=field)
    pp, c, proof = _PP[key], FL(T, LANES, "repeat", field), None
    for g in range(LANE_STEPS):
        c.advice = mont_rows(step_advice_ints(field, T, LANE_STEPS, LANES, g), m)
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z_of(field, LANES))
    assert proof.verify(pp, LANE_STEPS, z_of(field, LANES), z_of(field, LANES, T, LANE_STEPS)) is True
    return proof_bytes(pp, proof)


def test_three_lanes(ctx):
    field = FIELD_FQ
    _PP[(2, "lanes")] = pp = public_params_custom(ctx, FL(T, LANES, "repeat", field), field=field, custom_ahead=2)
    rb, n_cons, t = pp.repeat_rows()
    assert pp.repeat_lanes() == LANES and pp.early_rows() == (rb, LANES * n_cons * t)
    inv, j_base = walk_inv_and_j_base(field, LANES)
    chain = CustomChain.lanes_from_checkpoints(field, record_walk_body(minroot_body(field), field), inv, T, EVERY, LANE_STEPS, LANES,
                                               lanes_checkpoints(field, T, LANE_STEPS, EVERY, LANES), None, j_base)
    proof = NovaVDFProof.prove_recursively_custom(pp, FL(T, LANES, "repeat", field), chain, z_of(field, LANES), window_steps=100, check_steps=True)
    assert proof.ahead_stats() == (LANE_STEPS - 1, 0, 0)
    chain.free()
    assert proof_bytes(pp, proof) == lanes_reference(ctx)


# ---- b. a bad value -------------------------------------------------------------------------------------------------------------------
def test_a_value_outside_0_to_2_is_refused(ctx):
    with pytest.raises(VdfError) as e:
        public_params_custom(ctx, FC(T), custom_ahead=3)
    assert e.value.code == VDF_ERR_BAD_ARG and "tuning" in str(e.value)


# ---- d. misses ------------------------------------------------------------------------------------------------------------------------
def test_a_step_driven_by_another_chain_object_is_a_miss(ctx):
    pp, c, z0, proof = params(ctx, 2), FC(T), z0_of(FIELD_FQ), None
    a, b = chain_of(), chain_of()                      # the same checkpoints, two objects, two sets of traces
    a.materialize(ctx, 0, STEPS); b.materialize(ctx, 0, STEPS)
    for k in range(STEPS):
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, a if k < 3 else b, k, z0)
    assert proof.ahead_stats() == (STEPS - 2, 1, 0)    # step 3 found the rounds of (a, 3)
    assert proof.verify(pp, STEPS, z0, zi_of(FIELD_FQ, T, STEPS)) is True
    assert proof_bytes(pp, proof) == reference(ctx)
    a.free(); b.free()


@pytest.mark.parametrize("mode", [1, 2])
def test_an_inv_the_probe_did_not_see_is_a_miss_every_step(ctx, mode):
    """FCliar's inv is a variable of its own whose value is i_in + 1 in the probe and i_in in the step"""
    pp = params(ctx, mode, cls=FCliar)
    assert pp.early_rows() == (0, 0)                   # the repeat's rows read that variable: mode 2 is mode 1 here
    pp0, chain = params(ctx, 0, cls=FCliar), chain_of()
    proof = NovaVDFProof.prove_recursively_custom(pp, FCliar(T), chain, z0_of(FIELD_FQ), window_steps=100)
    assert proof.ahead_stats() == (0, STEPS - 1, 0)
    assert proof.verify(pp, STEPS, z0_of(FIELD_FQ), zi_of(FIELD_FQ, T, STEPS)) is True
    assert pp.digest() == pp0.digest()
    assert proof_bytes(pp, proof) == reference(ctx, cls=FCliar)
    chain.free()


# ---- e. step by step over pending walks ------------------------------------------------------------------------------------------------
def test_steps_driven_by_the_caller_over_pending_walks(ctx):
    pp, c, z0, proof = params(ctx, 2), FC(T), z0_of(FIELD_FQ), None
    chain = chain_of()
    chain.materialize(ctx, 0, 2, wait=True, launch_rounds=4)
    assert chain.materialize(ctx, 2, 3, wait=False, launch_rounds=4) == [0, 0, 0]
    for k in (0, 1):
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
    assert proof.ahead_stats() == (1, 0, 0)            # step 1's rounds were made during step 0; step 2's walks are pending
    assert proof.last_unsat() == (0, 2**64 - 1)
    chain.release(0, 2)
    chain.materialize(ctx, 5, 2, wait=False)
    for k in range(2, STEPS):
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
        assert proof.last_unsat() == (0, 2**64 - 1)    # under the next step's early rows, if there are any
    hits, misses, skipped = proof.ahead_stats()
    assert hits + misses + skipped == STEPS - 1 and misses == 0 and skipped >= 1
    # a probe is a witness synthesis with a trace too, and the only extra one: at most one per step
    assert all(w and adv is not None for w, adv in c.seen) and STEPS <= len(c.seen) <= 2 * STEPS
    assert proof.verify(pp, STEPS, z0, zi_of(FIELD_FQ, T, STEPS)) is True
    assert proof_bytes(pp, proof) == reference(ctx)
    chain.free()


# ---- f. errors keep their names ----------------------------------------------------------------------------------------------------------
def test_an_unsatisfied_row_is_named_as_under_the_default_tuning(ctx):
    said = []
    for mode in (0, 2):
        pp, chain = params(ctx, mode, cls=FW), chain_of()
        with pytest.raises(VdfError) as e:
            NovaVDFProof.prove_recursively_custom(pp, FW(T), chain, z0_of(FIELD_FQ), window_steps=3, check_steps=True)
        assert e.value.code == VDF_ERR_BAD_ARG and chain.memory() == (0, 0)
        said.append(str(e.value))
        chain.free()
    assert said[0] == said[1] and "step 0:" in said[0] and "(repetition 0, constraint 2 of the repeat)" in said[0]


def test_a_corrupted_checkpoint_names_its_step_and_the_context_goes_on(ctx):
    import ctypes as C
    from vdf_amd.minroot import nova_lib
    from vdf_amd.nova import _zn
    field, per = FIELD_FQ, T // EVERY
    pp = params(ctx, 2)
    wrong = checkpoints_of(minroot_chain(field, T, STEPS, X0, I0), 2, EVERY, MOD[field]).copy()
    wrong[2 * (3 * per + 2), 0] ^= np.uint64(1)        # step 3's middle checkpoint
    chain = chain_of(cps=wrong)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, FC(T), chain, z0_of(field), window_steps=2)
    assert e.value.code == VDF_ERR_BAD_ARG and "step 3:" in str(e.value) and "did not land" in str(e.value)
    assert chain.memory() == (0, 0)
    c, h = FC(T), C.c_void_p(1)
    assert nova_lib.vdf_nova_prove_recursively_custom(pp.handle, C.byref(c._c()), chain.handle, _zn(z0_of(field)), 2, 0, C.byref(h)) == VDF_ERR_BAD_ARG
    assert h.value is None
    chain.free()
    got, stats = recursively(ctx, 2, 2)                # a good chain on the same context and parameters
    assert got == reference(ctx) and stats[1] == 0


# ---- g. the plain step ------------------------------------------------------------------------------------------------------------------
def test_plain_steps_over_device_advice_are_left_alone(ctx):
    pp, c, z0, proof = params(ctx, 2), FC(T), z0_of(FIELD_FQ), None
    chain = chain_of()
    chain.materialize(ctx, 0, STEPS)
    for k in range(STEPS):
        c.advice = chain.advice(k)                     # a device address: the rounds run on the GPU, inside the step
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
    assert proof.ahead_stats() == (0, 0, 0) and len(c.seen) == STEPS
    assert proof_bytes(pp, proof) == reference(ctx)
    chain.free()
