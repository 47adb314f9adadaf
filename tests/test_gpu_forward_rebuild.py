"""GPU: traces rebuilt by forward tapes (vdf_round_tape_rebuild_lanes: k_tape_rebuild_lanes, k_tape_rebuild_lanes_tab) and the
ascending vdf_custom_chain above them.

a. the launcher against the host restatement, byte for byte, over the host file's matrix: entries, trace (its untouched parts
   still hold their fill pattern) and ok;
b. a planted wrong `expect` is a result, not an error;
c. both directions agree: the MinRoot forward round with the library's chain rebuilds the traces the inverse round walks down;
d. the chain: a Rescue-shaped circuit proved from its checkpoints is byte for byte the vdf_nova_prove_step_custom loop over host
   advice -- in lanes, in the other orientation, under custom_ahead = 2, and never with more than two windows and a spare;
e. a wrong checkpoint names its step and lane; f. VDF_CUSTOM_CHECK_STEPS names the row; g. the plain-C example, as a child process."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import forward_rebuild_spec as fs
import walks_spec
from pow_chain_spec import minroot_chain_body
from rounds_spec import MOD, mont_rows
from forward_rebuild_spec import EVERY, IDS, MATRIX, STEPS, case, run_window
from util import dev, dev_read, host
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.minroot import pow_chain as minroot_pow_chain
from vdf_amd.nova import (CHAIN_ASCENDING, CustomChain, NovaVDFProof, forward_tape_rebuild_eval_lanes, public_params_custom,
                          record_forward_body, record_walk_body, FIELD_FP, FIELD_FQ)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def filled(elems):
    import torch
    return torch.full((elems, 4), int(np.uint64(fs.FILL).astype(np.int64)), dtype=torch.int64, device="cuda")


def device_call(ctx):
    """forward_tape_rebuild_eval_lanes' signature over device tensors"""
    def call(field, tape, lanes, inv, entries, n, rounds, trace=None, expect=None, ok=None, **kw):
        ctx.round_tape_rebuild_lanes(field, tape, lanes, inv, entries, n, rounds, trace=trace, expect=expect, ok=ok, **kw)
    return call


# ---- a. launcher against restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,na,lanes,group,heads,tab", MATRIX, ids=IDS)
def test_the_launcher_is_the_restatement(ctx, field, na, lanes, group, heads, tab):
    import torch
    tape, inv, jb, chains, t = case(field, na, lanes, group, tab)
    lo, hi = fs.window(chains, na, t, EVERY, 0, STEPS)
    n, stride = STEPS * lanes * group, t + 2
    trace = np.full((n // group * stride * na, 4), fs.FILL, dtype="<u8")
    ok = np.full(n, -7, dtype="<i4")
    entries = run_window(forward_tape_rebuild_eval_lanes, field, tape, lanes, inv, jb, lo, hi, trace, ok, t, group, heads, stride)
    d_trace, d_ok = filled(trace.shape[0]), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_entries, base = dev(lo), 0
    call = device_call(ctx)
    for i, now in enumerate((2, 2, 1)):
        last = i == 2
        call(field, tape, lanes, inv, d_entries, n, now, trace=d_trace, walk_stride=EVERY, base=base, group=group, group_stride=stride, j_base=jb,
             j_group_step=t, heads=heads, expect=dev(hi) if last else None, ok=d_ok if last else None)
        base += now
    ctx.sync()
    assert host(d_entries).tobytes() == entries.tobytes() == hi.tobytes()
    assert d_ok.cpu().numpy().tolist() == ok.tolist() == [1] * n
    assert host(d_trace).tobytes() == trace.tobytes()
    assert trace.tobytes() == fs.window_traces(chains, na, t, 0, STEPS, stride, bool(heads)).tobytes()


def test_more_than_one_wavefront_and_a_partial_last_one(ctx):
    """130 walks of one group-less call (three wavefronts, the last of two lanes), lanes = 1, 7 rounds, no trace"""
    field, na, n = FIELD_FP, 2, 130
    m = MOD[field]
    tape = record_forward_body(fs.every_op_body(field, na), field)
    inv = mont_rows([5], m)
    start = mont_rows([int(v) for v in np.random.default_rng(3).integers(1, 2**62, size=n * na)], m)
    want = start.copy()
    forward_tape_rebuild_eval_lanes(field, tape, 1, inv, want, n, 7, walk_stride=9, base=1, group=0, j_base=[2**64 - 400], j_group_step=5)
    d = dev(start)
    ctx.round_tape_rebuild_lanes(field, tape, 1, inv, d, n, 7, walk_stride=9, base=1, group=0, j_base=[2**64 - 400], j_group_step=5)
    ctx.sync()
    assert host(d).tobytes() == want.tobytes()


# ---- b. a planted wrong expect -----------------------------------------------------------------------------------------------------
def test_a_planted_wrong_expect_is_a_result(ctx):
    import torch
    field, na, lanes, group = FIELD_FQ, 4, 3, 2
    tape, inv, jb, chains, t = case(field, na, lanes, group, True)
    lo, hi = fs.window(chains, na, t, EVERY, 0, STEPS)
    n = STEPS * lanes * group
    bad = hi.copy()
    bad[7 * na + 3, 2] ^= np.uint64(1)                 # the last column of walk 7's target
    d_entries, d_ok = dev(lo), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ctx.round_tape_rebuild_lanes(field, tape, lanes, inv, d_entries, n, EVERY, walk_stride=EVERY, group=group, group_stride=t + 1, j_base=jb,
                                 j_group_step=t, expect=dev(bad), ok=d_ok)
    ctx.sync()
    assert d_ok.cpu().numpy().tolist() == [int(w != 7) for w in range(n)]
    assert host(d_entries).tobytes() == hi.tobytes()


# ---- c. both directions agree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP], ids=["Fq", "Fp"])
def test_both_directions_rebuild_the_same_traces(ctx, field):
    """MinRoot at t = 16, every = 4, 3 steps: the forward round (x + y)^(1/5), x + j by the library's POWC chain, walked up, and
    the inverse round walked down by vdf_round_tape_walk under the same j_base"""
    m, t, every, steps, j_base = MOD[field], 16, 4, 3, 2**64 - 20
    fwd = record_forward_body(minroot_chain_body(field, minroot_pow_chain(field)), field)
    inv_tape, inv0 = record_walk_body(walks_spec.minroot_body(field), field), mont_rows([0], m)
    chain = fs.chain_trace(field, fwd, None, mont_rows([0x1234, 7], m), steps * t, j_base)
    lo, hi = fs.window([chain], 2, t, every, 0, steps)
    per, n = t // every, steps * (t // every)
    up, down = filled(steps * (t + 1) * 2), filled(steps * (t + 1) * 2)
    d_lo, d_hi = dev(lo), dev(hi)
    ctx.round_tape_rebuild_lanes(field, fwd, 1, None, d_lo, n, every, trace=up, walk_stride=every, base=0, group=per, group_stride=t + 1,
                                 j_base=[j_base], j_group_step=t, heads=True)
    ctx.round_tape_walk(field, inv_tape, inv0, d_hi, n, every, trace=down, walk_stride=every, top=every, group=per, group_stride=t + 1,
                        j_base=j_base, j_group_step=t, heads=True)
    ctx.sync()
    assert host(up).tobytes() == host(down).tobytes() == fs.window_traces([chain], 2, t, 0, steps, t + 1).tobytes()
    assert host(d_lo).tobytes() == hi.tobytes() and host(d_hi).tobytes() == lo.tobytes()


# ---- d. the chain ------------------------------------------------------------------------------------------------------------------
T_, EVERY_, STEPS_, ROWS_, WINDOW, LAUNCH = 8, 4, 5, 4, 2, 3
_PP = {}


@pytest.fixture(scope="module", autouse=True)
def free_the_parameter_sets():
    yield
    for pp in _PP.values():
        pp.free()
    _PP.clear()
    reference.cache_clear()


@functools.lru_cache(maxsize=None)
def table(field):
    return fs.rescue_table(field, ROWS_)


@functools.lru_cache(maxsize=None)
def forward_tape(field, wrong=False):
    return record_forward_body(fs.rescue_forward_body(field, table(field)[1], wrong), field)


@functools.lru_cache(maxsize=None)
def chains_of(field, lanes, wrong=False):
    """the lanes' whole chains from (0x51DE + l, 3 l), entry 0 without roots"""
    m = MOD[field]
    starts = mont_rows([v for l in range(lanes) for v in (0x51DE + l, 3 * l, 0, 0)], m)
    return fs.lane_chains(field, forward_tape(field, wrong), lanes, 0, None, starts, STEPS_ * T_, [0] * lanes)


def z_of(field, lanes, step, wrong=False):
    return [c[4 * step * T_ + k].tobytes() for c in chains_of(field, lanes, wrong) for k in range(2)]


def checkpoints(field, lanes, wrong=False):
    return np.concatenate([c.reshape(-1, 16)[::EVERY_].reshape(-1, 4) for c in chains_of(field, lanes, wrong)])


def circuit(field, lanes=1, probe=None):
    return fs.Rescue(T_, table(field)[1], field, lanes, probe)


def params(ctx, field=FIELD_FQ, lanes=1, **tune):
    key = (field, lanes, tuple(sorted(tune.items())))
    if key not in _PP:
        _PP[key] = public_params_custom(ctx, circuit(field, lanes), field=field, **tune)
    return _PP[key]


def chain_of(field, lanes=1, cps=None, wrong_tape=False):
    cps = checkpoints(field, lanes, wrong_tape) if cps is None else cps
    if lanes == 1:
        chain = CustomChain.from_checkpoints(field, forward_tape(field, wrong_tape), None, T_, EVERY_, STEPS_, cps, forward=True)
    else:
        chain = CustomChain.lanes_from_checkpoints(field, forward_tape(field, wrong_tape), None, T_, EVERY_, STEPS_, lanes, cps, forward=True)
    chain.set_launch_rounds(LAUNCH)                    # prove_recursively_custom asks for 0: slices of 3 + 1 rounds
    assert chain.direction == CHAIN_ASCENDING and chain.launch_rounds(0) == LAUNCH
    return chain


@functools.lru_cache(maxsize=None)
def reference(ctx, field=FIELD_FQ, lanes=1):
    """the proof bytes of vdf_nova_prove_step_custom step by step over HOST advice under the default tuning; verified"""
    pp, c, proof = params(ctx, field, lanes), circuit(field, lanes), None
    for g in range(STEPS_):
        c.advice = fs.step_advice(chains_of(field, lanes), 4, T_, g)
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z_of(field, lanes, 0))
    assert proof.verify(pp, STEPS_, z_of(field, lanes, 0), z_of(field, lanes, STEPS_)) is True
    out = proof.serialize()
    proof.free()
    return out


def test_the_ascending_chain_gives_the_plain_loops_proof(ctx):
    field = FIELD_FQ
    pp, chain = params(ctx, field), chain_of(field)
    z0, zi = z_of(field, 1, 0), z_of(field, 1, STEPS_)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z0, window_steps=WINDOW, check_steps=True)
    assert proof.num_steps() == STEPS_ and proof.serialize() == reference(ctx, field)
    assert proof.verify(pp, STEPS_, z0, zi) is True
    snark = proof.compress(pp)
    assert snark.verify(pp, STEPS_, z0, zi) is True
    assert chain.memory() == (0, ROWS_ * 2 * 32)       # no trace is left; the table's device copy lives with the chain
    snark.free(); proof.free(); chain.free()


def test_the_traces_a_window_holds_are_the_chains(ctx):
    """materialize alone, in slices of 3 + 1: step 1 .. 3 of three lanes, entries 0 .. t of each lane"""
    field, L = FIELD_FQ, 3
    chain = chain_of(field, L)
    assert chain.materialize(ctx, 1, 3, wait=True) == [0, 0, 0]
    for g in (1, 2, 3):
        got = dev_read(ctx, chain.advice(g), L * (T_ + 1) * 4 * 32)
        assert got.tobytes() == fs.step_advice(chains_of(field, L), 4, T_, g).tobytes()
    assert chain.advice(0) is None and chain.memory()[0] == 3
    chain.release(1, 3)
    chain.free()


def test_three_lanes(ctx):
    field, L = FIELD_FQ, 3
    pp, chain = params(ctx, field, L), chain_of(field, L)
    z0, zi = z_of(field, L, 0), z_of(field, L, STEPS_)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field, L), chain, z0, window_steps=WINDOW, check_steps=True)
    assert proof.serialize() == reference(ctx, field, L)
    assert proof.verify(pp, STEPS_, z0, zi) is True
    snark = proof.compress(pp)
    assert snark.verify(pp, STEPS_, z0, zi) is True
    snark.free(); proof.free(); chain.free()


def test_the_other_orientation(ctx):
    field = FIELD_FP
    pp, chain = params(ctx, field), chain_of(field)
    z0, zi = z_of(field, 1, 0), z_of(field, 1, STEPS_)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z0, window_steps=WINDOW, check_steps=True)
    assert proof.serialize() == reference(ctx, field)
    assert proof.verify(pp, STEPS_, z0, zi) is True
    snark = proof.compress(pp)
    assert snark.verify(pp, STEPS_, z0, zi) is True
    snark.free(); proof.free(); chain.free()


def test_the_lookahead_runs_above_an_ascending_chain(ctx):
    field = FIELD_FQ
    pp, chain = params(ctx, field, custom_ahead=2), chain_of(field)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z_of(field, 1, 0), window_steps=WINDOW)
    hits, misses, _ = proof.ahead_stats()
    assert proof.serialize() == reference(ctx, field) and hits > 0 and misses == 0
    proof.free(); chain.free()


def test_never_more_than_two_windows_and_a_spare(ctx):
    field = FIELD_FQ
    pp, chain = params(ctx, field), chain_of(field)
    seen = []
    c = circuit(field, probe=lambda: seen.append(chain.memory()))
    proof = NovaVDFProof.prove_recursively_custom(pp, c, chain, z_of(field, 1, 0), window_steps=WINDOW)
    window, tab = WINDOW * (T_ + 1) * 4 * 32, ROWS_ * 2 * 32
    assert len(seen) == STEPS_ and max(n for n, _ in seen) == 2 * WINDOW
    assert all(n <= 2 * WINDOW and b <= 3 * window + tab for n, b in seen)
    assert chain.memory() == (0, tab)
    proof.free(); chain.free()


# ---- e. a wrong checkpoint ---------------------------------------------------------------------------------------------------------
def test_a_wrong_checkpoint_names_its_step_and_lane(ctx):
    import ctypes as C
    from vdf_amd.minroot import nova_lib
    from vdf_amd.nova import _zn
    field, L, per = FIELD_FQ, 3, T_ // EVERY_
    pp = params(ctx, field, L)
    wrong = checkpoints(field, L).copy()
    # lane 1's checkpoint ABOVE the first interval of step 3 (the second window at W = 2): its third column
    wrong[4 * (1 * (STEPS_ * per + 1) + 3 * per + 1) + 2, 0] ^= np.uint64(1)
    chain = chain_of(field, L, cps=wrong)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, circuit(field, L), chain, z_of(field, L, 0), window_steps=WINDOW)
    assert e.value.code == VDF_ERR_BAD_ARG and "step 3, lane 1: a walk did not land on the checkpoint above it" in str(e.value)
    assert chain.memory() == (0, ROWS_ * 2 * 32)       # nothing is left in flight, no trace stays
    c, h = circuit(field, L), C.c_void_p(1)
    assert nova_lib.vdf_nova_prove_recursively_custom(pp.handle, C.byref(c._c()), chain.handle, _zn(z_of(field, L, 0)), WINDOW, 0, C.byref(h)) == VDF_ERR_BAD_ARG
    assert h.value is None
    chain.free()
    # one lane: no lane in the message; and the context and the parameters still work
    wrong = checkpoints(field, 1).copy()
    wrong[4 * 2 + 1, 1] ^= np.uint64(1)
    chain = chain_of(field, cps=wrong)
    with pytest.raises(VdfError) as e:
        chain.materialize(ctx, 0, STEPS_)
    assert "step 0: a walk did not land on the checkpoint above it" in str(e.value) and chain.last_bad == [1, 1, 0, 0, 0]
    chain.free()
    good = chain_of(field)
    proof = NovaVDFProof.prove_recursively_custom(params(ctx, field), circuit(field), good, z_of(field, 1, 0), window_steps=WINDOW)
    assert proof.serialize() == reference(ctx, field)
    proof.free(); good.free()


# ---- f. VDF_CUSTOM_CHECK_STEPS -----------------------------------------------------------------------------------------------------
def test_a_forward_tape_that_disagrees_with_the_round_body_is_named_by_its_row(ctx):
    """the wrong tape adds 1 to s0' (its own checkpoints agree with it): the carry the round body computes from entry 1's roots is
    not the state entry 2's roots are the roots of, so repetition 1's first enforce, r0^5 = s0, fails"""
    field = FIELD_FQ
    pp = params(ctx, field)
    chain = chain_of(field, wrong_tape=True)
    z0 = z_of(field, 1, 0, wrong=True)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z0, window_steps=WINDOW, check_steps=True)
    text = str(e.value)
    assert e.value.code == VDF_ERR_BAD_ARG and "step 0:" in text and "unsatisfied rows, first row" in text
    rb, n_cons, _ = pp.repeat_rows()
    first = int(text.split("first row ")[1].split(" ")[0])
    assert first == rb + 1 * n_cons + 2 and "(repetition 1, constraint 2 of the repeat)" in text
    chain.free()


# ---- g. the C example --------------------------------------------------------------------------------------------------------------
def test_the_c_example_proves_a_rescue_chain(ctx):
    exe = os.path.join(ROOT, "examples", "prove_rescue_chain")
    assert os.path.exists(exe), "examples/prove_rescue_chain is built by vdf_amd/csrc/Makefile (all)"
    src = open(exe + ".c").read()
    # no inverse tape anywhere in the file: nothing is recorded as a walk body, and no descending constructor or walk is called
    assert "vdf_nova_walk_body_record" not in src and "vdf_round_tape_walk" not in src and "_from_checkpoints(" not in src
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(T_), str(EVERY_), str(STEPS_), str(ROWS_), str(0x51DE)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true"
    field = FIELD_FQ
    pp, chain = params(ctx, field), chain_of(field)
    assert int(lines["digest"], 16) == pp.digest()
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z_of(field, 1, 0), window_steps=WINDOW)
    snark = proof.compress(pp)
    assert lines["compressed proof sha256"] == hashlib.sha256(snark.serialize()).hexdigest()
    snark.free(); proof.free(); chain.free()
