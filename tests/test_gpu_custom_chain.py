"""GPU: a custom circuit's chain proved from its checkpoints (include/vdf_nova.h vdf_custom_chain, vdf_nova_prove_step_custom_chain,
vdf_nova_prove_recursively_custom).

a. the traces materialize builds are byte for byte the host restatement's (vdf_nova_walk_tape_eval, one uncut call): walks cut
   into launches of 4 rounds, one-round walks at the wavefront boundary, one walk per step, three columns, a counter that wraps
   inside the window, both fields; a neighbouring range is not disturbed;
b. wait = 0: the prover's steps pump the walks, traces and proof are those of wait = 1;
c. the running proof and the compressed proof are byte for byte those of the vdf_nova_prove_step_custom loop over host advice, for
   every window length, with periodic rows, in the other orientation, and from a DEVICE checkpoint array;
d. never more than two windows (and one spare allocation) of traces, and none after the call;
e. a corrupted checkpoint names its step, leaves *proof NULL and the context working;
f. the refusals; g. the plain-C example, as a fresh child process."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

from custom_chain_spec import (FC, FW, I0, X0, checkpoints_of, every_op_chain, forward_minroot_body, minroot_chain, step_traces, z0_of,
                               zi_of)
from rounds_spec import MOD, mont_rows
from util import dev_read
from walks_spec import every_op_body, minroot_body
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.nova import (CustomChain, NovaVDFProof, custom_chain_window_host, public_params_custom, record_forward_body,
                          record_walk_body, shape_digest_custom, FIELD_FP, FIELD_FQ)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, EVERY, STEPS = 65, 13, 7
_PP = {}


@pytest.fixture(scope="module", autouse=True)
def free_the_parameter_sets():
    """the module's parameter sets go with the module: their compression queues come from the device's pool, and what a later test
    file finds there is not this one's business"""
    yield
    for pp in _PP.values():
        pp.free()
    _PP.clear()
    reference.cache_clear()


def params(ctx, field=FIELD_FQ, t=T, periodic=0, cls=FC):
    """one parameter set per shape for the whole module"""
    key = (field, t, periodic, cls.__name__)
    if key not in _PP:
        _PP[key] = public_params_custom(ctx, cls(t, field), field=field, periodic_rows=periodic)
    return _PP[key]


def minroot_parts(field, t=T, every=EVERY, steps=STEPS, x0=X0, i0=I0):
    m = MOD[field]
    return record_walk_body(minroot_body(field), field), mont_rows([i0], m), checkpoints_of(minroot_chain(field, t, steps, x0, i0), 2, every, m)


def minroot_chain_obj(field, t=T, every=EVERY, steps=STEPS, cps=None, x0=X0, i0=I0):
    tape, inv, good = minroot_parts(field, t, every, steps, x0, i0)
    return CustomChain.from_checkpoints(field, tape, inv, t, every, steps, good if cps is None else cps)


def trace_bytes(ctx, chain, k):
    p = chain.advice(k)
    assert p, "step %d has no trace" % k
    return dev_read(ctx, p, (chain.t + 1) * chain.n_adv * 32).tobytes()


def check_window(ctx, chain, field, tape, inv, cps, first, count, j_base=0):
    """steps [first, first + count) of the chain against ONE uncut host call"""
    want, _, ok = custom_chain_window_host(field, tape, inv, chain.t, chain.every, cps, first, count, j_base, chain.every)
    assert ok.all()
    per_step = (chain.t + 1) * chain.n_adv
    for g in range(count):
        assert trace_bytes(ctx, chain, first + g) == want[g * per_step:(g + 1) * per_step].tobytes(), "step %d" % (first + g)


@functools.lru_cache(maxsize=None)
def reference(ctx, field, periodic=0, t=T, steps=STEPS, x0=X0, i0=I0):
    """(running proof bytes, compressed proof bytes) of the plain loop: vdf_nova_prove_step_custom step by step over HOST advice"""
    pp, c, proof = params(ctx, field, t, periodic), FC(t, field), None
    for tr in step_traces(field, t, steps, x0, i0):
        c.advice = tr
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0_of(field, x0, i0))
    assert proof.verify(pp, steps, z0_of(field, x0, i0), zi_of(field, t, steps, x0, i0)) is True
    snark = proof.compress(pp)
    out = proof.serialize(), snark.serialize()
    snark.free(); proof.free()
    return out


def proof_bytes(pp, proof):
    snark = proof.compress(pp)
    out = proof.serialize(), snark.serialize()
    snark.free(); proof.free()
    return out


# ---- a. traces ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_traces_of_a_window_cut_into_launches_of_four_rounds(ctx, field):
    tape, inv, cps = minroot_parts(field)
    chain = CustomChain.from_checkpoints(field, tape, inv, T, EVERY, STEPS, cps)
    assert chain.materialize(ctx, 0, 3, wait=True, launch_rounds=4) == [0, 0, 0]
    assert chain.memory() == (3, 3 * (T + 1) * 2 * 32)
    check_window(ctx, chain, field, tape, inv, cps, 0, 3)
    assert chain.advice(3) is None and chain.advice(6) is None
    # the entries are the chain's own, by the oracle's evaluator
    e = minroot_chain(field, T, STEPS)
    assert trace_bytes(ctx, chain, 1) == mont_rows(e[2 * T:2 * (2 * T + 1)], MOD[field]).tobytes()
    chain.release(0, 3)
    assert chain.memory() == (0, 0)
    chain.free()


@pytest.mark.parametrize("t", [63, 64, 65])
def test_one_round_walks_at_the_wavefront_boundary(ctx, t):
    """every = 1 and a one-step window: t walks of one round"""
    field = FIELD_FQ
    tape, inv, cps = minroot_parts(field, t, 1, 3)
    chain = CustomChain.from_checkpoints(field, tape, inv, t, 1, 3, cps)
    assert chain.materialize(ctx, 1, 1) == [0]
    check_window(ctx, chain, field, tape, inv, cps, 1, 1)
    assert chain.memory() == (1, (t + 1) * 64)
    chain.free()


def test_one_walk_per_step_and_a_neighbouring_range(ctx):
    """every = t; ranges materialised one after the other leave each other's traces alone, also when one is built again"""
    field = FIELD_FQ
    tape, inv, cps = minroot_parts(field, T, T, STEPS)
    chain = CustomChain.from_checkpoints(field, tape, inv, T, T, STEPS, cps)
    chain.materialize(ctx, 2, 3)
    mid = [trace_bytes(ctx, chain, k) for k in (2, 3, 4)]
    chain.materialize(ctx, 0, 2)
    chain.materialize(ctx, 5, 2, launch_rounds=7)
    check_window(ctx, chain, field, tape, inv, cps, 0, 2)
    check_window(ctx, chain, field, tape, inv, cps, 2, 3)
    check_window(ctx, chain, field, tape, inv, cps, 5, 2)
    chain.release(0, 2); chain.release(5, 2)
    chain.materialize(ctx, 0, 7)                       # [0, 2) and [5, 7) again, around the resident range: one block from 0 to 6
    assert chain.memory()[0] == 7
    check_window(ctx, chain, field, tape, inv, cps, 0, 7)
    assert [trace_bytes(ctx, chain, k) for k in (2, 3, 4)] == mid
    chain.free()


@pytest.mark.parametrize("j_base", [0, 2**64 - 12])
def test_three_columns_and_a_counter_that_wraps_inside_the_window(ctx, j_base):
    field, t, every, steps = FIELD_FP, 10, 5, 4
    m = MOD[field]
    tape = record_walk_body(every_op_body(field), field)
    inv_ints, cp_ints = every_op_chain(field, t, steps, every, j_base)
    inv, cps = mont_rows(inv_ints, m), mont_rows(cp_ints, m)
    chain = CustomChain.from_checkpoints(field, tape, inv, t, every, steps, cps, j_base=j_base)
    assert chain.materialize(ctx, 0, 3, launch_rounds=2) == [0, 0, 0]       # j runs over 2^64 - 12 .. 2^64 + 17
    check_window(ctx, chain, field, tape, inv, cps, 0, 3, j_base)
    assert chain.materialize(ctx, 3, 1) == [0]
    check_window(ctx, chain, field, tape, inv, cps, 3, 1, j_base)
    chain.free()


# ---- b. wait = 0 -------------------------------------------------------------------------------------------------------------
def test_walks_enqueued_without_waiting_are_pumped_by_the_prover(ctx):
    field = FIELD_FQ
    pp, c = params(ctx, field), FC(T, field)
    tape, inv, cps = minroot_parts(field)
    chain = CustomChain.from_checkpoints(field, tape, inv, T, EVERY, STEPS, cps)
    z0, proof = z0_of(field), None
    chain.materialize(ctx, 0, 2, wait=True, launch_rounds=4)
    assert chain.materialize(ctx, 2, 3, wait=False, launch_rounds=4) == [0, 0, 0]
    for k in (0, 1):                                   # each step pumps its share of the 13 - 4 rounds that are left
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
    check_window(ctx, chain, field, tape, inv, cps, 2, 3)
    chain.release(0, 2)
    chain.materialize(ctx, 5, 2, wait=False)
    for k in range(2, STEPS):
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
    assert all(w and a is not None for w, a in c.seen)  # every witness synthesis was handed a trace
    assert proof.verify(pp, STEPS, z0, zi_of(field, T, STEPS)) is True
    assert proof_bytes(pp, proof) == reference(ctx, field)
    chain.free()


# ---- c. proof bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_steps", [2, 3, 7, 100, 0, 1])
def test_the_proof_is_the_plain_loops_for_every_window_length(ctx, window_steps):
    field = FIELD_FQ
    pp, chain = params(ctx, field), minroot_chain_obj(field)
    proof = NovaVDFProof.prove_recursively_custom(pp, FC(T, field), chain, z0_of(field), window_steps=window_steps)
    assert proof.num_steps() == STEPS and chain.memory() == (0, 0)
    assert proof_bytes(pp, proof) == reference(ctx, field)
    chain.free()


def test_the_proof_with_periodic_rows(ctx):
    field = FIELD_FQ
    pp, chain = params(ctx, field, periodic=1), minroot_chain_obj(field)
    assert pp.periodic_rows() is not None and pp.stencil() == 7
    proof = NovaVDFProof.prove_recursively_custom(pp, FC(T, field), chain, z0_of(field), window_steps=3, check_steps=True)
    assert proof_bytes(pp, proof) == reference(ctx, field, 1) == reference(ctx, field, 0)
    chain.free()


def test_the_proof_in_the_other_orientation(ctx):
    field = FIELD_FP
    pp, chain = params(ctx, field), minroot_chain_obj(field)
    proof = NovaVDFProof.prove_recursively_custom(pp, FC(T, field), chain, z0_of(field), window_steps=3)
    assert proof_bytes(pp, proof) == reference(ctx, field)
    chain.free()


def test_the_proof_from_a_device_checkpoint_array(ctx):
    """two chains evaluated on the device (vdf_round_tape_eval_batch); chain 1's slice of the output is the constructor's input"""
    import torch
    field, m, per = FIELD_FQ, MOD[FIELD_FQ], T // EVERY
    fwd = record_forward_body(forward_minroot_body(field), field)
    n_cp = STEPS * per + 1
    d_out = torch.zeros((2 * n_cp * 2, 4), dtype=torch.int64, device="cuda")
    ctx.round_tape_eval_batch(field, fwd, mont_rows([I0], m), mont_rows([X0, 0, X0 + 1, 0], m), 2, STEPS * T, d_out, every=EVERY)
    ctx.sync()
    tape, inv, _ = minroot_parts(field)
    chain = CustomChain.from_checkpoints(field, tape, inv, T, EVERY, STEPS, d_out.data_ptr() + n_cp * 2 * 32)
    assert d_out[n_cp * 2:].cpu().numpy().view("<u8").tobytes() == minroot_parts(field, x0=X0 + 1)[2].tobytes()
    pp = params(ctx, field)
    proof = NovaVDFProof.prove_recursively_custom(pp, FC(T, field), chain, z0_of(field, X0 + 1), window_steps=4)
    assert proof_bytes(pp, proof) == reference(ctx, field, x0=X0 + 1)
    chain.free()


# ---- d. two windows at most ----------------------------------------------------------------------------------------------------
def test_never_more_than_two_windows_of_traces(ctx):
    field, W = FIELD_FQ, 2
    pp, chain = params(ctx, field), minroot_chain_obj(field)
    seen = []
    c = FC(T, field, probe=lambda: seen.append(chain.memory()))
    proof = NovaVDFProof.prove_recursively_custom(pp, c, chain, z0_of(field), window_steps=W)
    window = W * (T + 1) * 2 * 32
    assert len(seen) == STEPS and max(n for n, _ in seen) == 2 * W
    assert all(n <= 2 * W and b <= 2 * window + window for n, b in seen)
    assert chain.memory() == (0, 0)
    proof.free(); chain.free()


# ---- e. a corrupted checkpoint ---------------------------------------------------------------------------------------------------
def test_a_corrupted_checkpoint_names_its_step(ctx):
    field, per = FIELD_FQ, T // EVERY
    pp = params(ctx, field)
    wrong = minroot_parts(field)[2].copy()
    wrong[2 * (3 * per + 2), 0] ^= np.uint64(1)        # step 3's middle checkpoint: two walks of step 3 touch it, the second window at W = 2
    chain = minroot_chain_obj(field, cps=wrong)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, FC(T, field), chain, z0_of(field), window_steps=2)
    assert e.value.code == VDF_ERR_BAD_ARG and "step 3:" in str(e.value) and "did not land" in str(e.value)
    assert chain.memory() == (0, 0)
    # *proof = NULL, through the C ABI
    import ctypes as C
    from vdf_amd.minroot import nova_lib
    from vdf_amd.nova import _zn
    c, h = FC(T, field), C.c_void_p(1)
    assert nova_lib.vdf_nova_prove_recursively_custom(pp.handle, C.byref(c._c()), chain.handle, _zn(z0_of(field)), 2, 0, C.byref(h)) == VDF_ERR_BAD_ARG
    assert h.value is None
    # the same corruption through materialize alone
    with pytest.raises(VdfError):
        chain.materialize(ctx, 0, STEPS)
    assert chain.last_bad == [0, 0, 0, 1, 0, 0, 0] and chain.memory()[0] == STEPS - 1 and chain.advice(3) is None
    chain.free()
    # a second, valid call with the same context and parameters
    good = minroot_chain_obj(field)
    proof = NovaVDFProof.prove_recursively_custom(pp, FC(T, field), good, z0_of(field), window_steps=2)
    assert proof.verify(pp, STEPS, z0_of(field), zi_of(field, T, STEPS)) is True
    assert proof_bytes(pp, proof) == reference(ctx, field)
    good.free()


# ---- f. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    field = FIELD_FQ
    pp, c, z0 = params(ctx, field), FC(T, field), z0_of(field)
    chain = minroot_chain_obj(field)

    def refused(what, circuit=c, ch=chain, k=0, proof=None):
        with pytest.raises(VdfError) as e:
            NovaVDFProof.prove_step_custom_chain(pp, proof, circuit, ch, k, z0)
        assert e.value.code == VDF_ERR_BAD_ARG and what in str(e.value), str(e.value)
    refused("advice of step 0 not materialised")
    chain.materialize(ctx, 0, 2)
    refused("beyond the chain", k=STEPS)
    other = minroot_chain_obj(FIELD_FP)
    refused("the chain is over Fp", ch=other)
    other.free()
    short = minroot_chain_obj(field, t=13, every=13, steps=2)       # a trace shorter than the repeat reads
    refused("differs from the vdf_cs_repeat", ch=short)
    short.free()
    refused("differs from the one these parameters were made with", circuit=FW(T, field))     # the existing refusal, through the new call
    proof = NovaVDFProof.prove_step_custom_chain(pp, None, c, chain, 0, z0)
    refused("out of order", k=0, proof=proof)
    refused("out of order", k=2, proof=proof)
    proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, 1, z0)
    refused("advice of step 2 not materialised", k=2, proof=proof)
    assert proof.num_steps() == 2
    proof.free(); chain.free()


# ---- g. the C example ----------------------------------------------------------------------------------------------------------
def test_the_c_example_proves_a_chain(ctx):
    exe = os.path.join(ROOT, "examples", "prove_custom_chain")
    assert os.path.exists(exe), "examples/prove_custom_chain is built by vdf_amd/csrc/Makefile (all)"
    t, every, steps, window, x0 = 65, 13, 5, 2, 123
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(t), str(every), str(steps), str(window), str(x0)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true"
    assert lines["resident after the proof"] == "0 steps, 0 bytes"
    assert int(lines["digest"], 16) == shape_digest_custom(FC(t))[0]
    pp, chain = params(ctx, FIELD_FQ), minroot_chain_obj(FIELD_FQ, t, every, steps, x0=x0, i0=0)
    proof = NovaVDFProof.prove_recursively_custom(pp, FC(t), chain, z0_of(FIELD_FQ, x0, 0), window_steps=window, check_steps=True)
    assert lines["compressed proof sha256"] == hashlib.sha256(proof_bytes(pp, proof)[1]).hexdigest()
    assert pp.digest() == int(lines["digest"], 16)
    chain.free()
