"""GPU: custom chains that grow, and vdf_nova_eval_and_prove_custom above them (include/vdf_nova.h CHAINS THAT GROW).

The reference bytes in every case are the vdf_nova_prove_step_custom loop over HOST advice.  Shapes: t = 8, every = 4, 5 steps, a
table of 4 rows, launch_rounds 3 (a walk is two slices), lanes 1 and 3; the Rescue-shaped circuit of forward_rebuild_spec (4 columns,
ascending) and MinRoot through the seam (custom_chain_spec / custom_lanes_spec: 2 columns, descending).

1. step-by-step growth by every hand-over; 2. three lanes, the other orientation; 3. the trace bytes materialize leaves; 4. a step not
yet pushed is beyond the chain; 5. the whole-chain prover over a chain pushed completely; 6. custom_ahead = 2 over a chain grown one
step ahead of the prover; 7. eval_and_prove_custom; 8. the plain-C example, as a child process."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import forward_rebuild_spec as fs
from custom_chain_spec import FC, I0, X0, checkpoints_of, forward_minroot_body, minroot_chain, step_traces, z0_of, zi_of
from custom_lanes_spec import FL, lane_entries, step_advice_ints, walk_inv_and_j_base
from custom_lanes_spec import z_of as minroot_lanes_z
from rounds_spec import MOD, mont_rows
from util import dev_read
from walks_spec import minroot_body
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.nova import (CHAIN_ASCENDING, CHAIN_DESCENDING, CustomChain, NovaVDFProof, public_params_custom, record_forward_body,
                          record_walk_body, FIELD_FP, FIELD_FQ)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, EVERY, STEPS, ROWS, LAUNCH = 8, 4, 5, 4, 3
PER = T // EVERY
_PP = {}


@pytest.fixture(scope="module", autouse=True)
def free_the_parameter_sets():
    yield
    for pp in _PP.values():
        pp.free()
    _PP.clear()
    reference.cache_clear()


# ---- the two circuits behind one face: kind = "rescue" (ascending, 4 columns) / "minroot" (descending, 2 columns) ------------------
@functools.lru_cache(maxsize=None)
def table(field):
    return fs.rescue_table(field, ROWS)


@functools.lru_cache(maxsize=None)
def tapes(kind, field):
    """(the forward tape, the tape a chain of checkpoints rebuilds with, its direction)"""
    if kind == "rescue":
        f = record_forward_body(fs.rescue_forward_body(field, table(field)[1]), field)
        return f, f, CHAIN_ASCENDING
    return record_forward_body(forward_minroot_body(field), field), record_walk_body(minroot_body(field), field), CHAIN_DESCENDING


def n_adv(kind):
    return 4 if kind == "rescue" else 2


def inv_and_j_base(kind, field, lanes):
    if kind == "rescue":
        return None, [0] * lanes
    return walk_inv_and_j_base(field, lanes)           # the same pair serves the forward tape: y' = x + inv + J either way


@functools.lru_cache(maxsize=None)
def chains_of(kind, field, lanes):
    """the lanes' whole chains, uint64[(STEPS T + 1) n_adv, 4] each, from the specs' own evaluators"""
    m = MOD[field]
    if kind == "rescue":
        starts = mont_rows([v for l in range(lanes) for v in (0x51DE + l, 3 * l, 0, 0)], m)
        return fs.lane_chains(field, tapes(kind, field)[0], lanes, 0, None, starts, STEPS * T, [0] * lanes)
    return [mont_rows(lane_entries(field, T, STEPS, l), m) for l in range(lanes)]       # oracle/pasta.py integers


def advice_of(kind, field, lanes, g):
    return fs.step_advice(chains_of(kind, field, lanes), n_adv(kind), T, g)


def checkpoints_of_step(kind, field, lanes, g):
    na = n_adv(kind)
    return np.concatenate([c[g * T * na:(g * T + T + 1) * na].reshape(-1, 4 * na)[::EVERY].reshape(-1, 4) for c in chains_of(kind, field, lanes)])


def initial_of(kind, field, lanes):
    return np.concatenate([c[:n_adv(kind)] for c in chains_of(kind, field, lanes)])


def final_of(kind, field, lanes):
    return np.concatenate([c[-n_adv(kind):] for c in chains_of(kind, field, lanes)])


def z_of(kind, field, lanes, step):
    if kind == "rescue":
        return [c[4 * step * T + k].tobytes() for c in chains_of(kind, field, lanes) for k in range(2)]
    if lanes == 1:
        return zi_of(field, T, step) if step else z0_of(field)
    return minroot_lanes_z(field, lanes, T, step)


def circuit(kind, field, lanes=1):
    if kind == "rescue":
        return fs.Rescue(T, table(field)[1], field, lanes)
    return FC(T, field) if lanes == 1 else FL(T, lanes, "repeat", field)


def params(ctx, kind, field=FIELD_FQ, lanes=1, **tune):
    key = (kind, field, lanes, tuple(sorted(tune.items())))
    if key not in _PP:
        _PP[key] = public_params_custom(ctx, circuit(kind, field, lanes), field=field, **tune)
    return _PP[key]


@functools.lru_cache(maxsize=None)
def reference(ctx, kind, field=FIELD_FQ, lanes=1):
    """the proof bytes of vdf_nova_prove_step_custom step by step over HOST advice under the default tuning; verified"""
    pp, c, proof = params(ctx, kind, field, lanes), circuit(kind, field, lanes), None
    for g in range(STEPS):
        c.advice = advice_of(kind, field, lanes, g)
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z_of(kind, field, lanes, 0))
    assert proof.verify(pp, STEPS, z_of(kind, field, lanes, 0), z_of(kind, field, lanes, STEPS)) is True
    out = proof.serialize()
    proof.free()
    return out


def begin(kind, field, lanes, handover):
    """an empty chain; a chain of whole traces is given the forward tape when it has no walk tape of its own to show"""
    _, rebuild, direction = tapes(kind, field)
    inv, jb = inv_and_j_base(kind, field, lanes)
    chain = CustomChain.begin(field, rebuild, direction, inv, T, initial_of(kind, field, lanes), lanes, jb)
    chain.set_launch_rounds(LAUNCH)
    assert len(chain) == 0 and chain.direction == direction and chain.memory() == (0, 0)
    return chain


def push(chain, kind, field, lanes, handover, g):
    if handover == "advice":
        chain.push_advice(advice_of(kind, field, lanes, g))
    else:
        chain.push_checkpoints(EVERY, checkpoints_of_step(kind, field, lanes, g))


def table_bytes(kind, handover):
    """the device copy of a table, made by the first walks of a chain that has one (no walks: no copy)"""
    return ROWS * 2 * 32 if kind == "rescue" and handover == "checkpoints" else 0


def grown_step_by_step(ctx, kind, field, lanes, handover):
    pp, c, chain, proof = params(ctx, kind, field, lanes), circuit(kind, field, lanes), begin(kind, field, lanes, handover), None
    z0, zi = z_of(kind, field, lanes, 0), z_of(kind, field, lanes, STEPS)
    at_begin = chain.host_bytes()
    for k in range(STEPS):
        push(chain, kind, field, lanes, handover, k)
        assert len(chain) == k + 1
        assert chain.materialize(ctx, k, 1, wait=False) == [0]
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
        chain.release(k, 1)
    assert proof.num_steps() == STEPS and proof.serialize() == reference(ctx, kind, field, lanes)
    assert proof.verify(pp, STEPS, z0, zi) is True
    snark = proof.compress(pp)
    assert snark.verify(pp, STEPS, z0, zi) is True
    assert chain.memory() == (0, table_bytes(kind, handover))                       # no trace is left
    grew = STEPS * lanes * PER * n_adv(kind) * 32 if handover == "checkpoints" else 0     # released advice leaves nothing behind
    assert chain.host_bytes() == at_begin + grew
    snark.free(); proof.free(); chain.free()


# ---- 1. step-by-step growth --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,handover", [("minroot", "checkpoints"), ("rescue", "checkpoints"), ("rescue", "advice"), ("minroot", "advice")],
                         ids=["checkpoints descending", "checkpoints ascending", "advice", "advice over a walk tape"])
def test_a_chain_grown_step_by_step_gives_the_plain_loops_proof(ctx, kind, handover):
    grown_step_by_step(ctx, kind, FIELD_FQ, 1, handover)


# ---- 2. three lanes, the other orientation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,handover", [("rescue", "checkpoints"), ("rescue", "advice"), ("minroot", "checkpoints")],
                         ids=["checkpoints ascending", "advice", "checkpoints descending"])
def test_three_lanes(ctx, kind, handover):
    grown_step_by_step(ctx, kind, FIELD_FQ, 3, handover)


def test_the_other_orientation(ctx):
    grown_step_by_step(ctx, "rescue", FIELD_FP, 1, "checkpoints")


# ---- 3. trace bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handover", ["advice", "checkpoints"])
def test_the_traces_materialize_leaves(ctx, handover):
    kind, field, L = "rescue", FIELD_FQ, 3
    chain = begin(kind, field, L, handover)
    nbytes = L * (T + 1) * 4 * 32
    for g in range(3):
        push(chain, kind, field, L, handover, g)
    assert chain.materialize(ctx, 0, 2, wait=False) == [0, 0]                     # two steps in one job, not waited for ...
    assert chain.materialize(ctx, 2, 1, wait=True) == [0]                         # ... and one more, which resolves them first
    for g in range(3):
        assert dev_read(ctx, chain.advice(g), nbytes).tobytes() == advice_of(kind, field, L, g).tobytes(), "step %d" % g
    assert chain.memory() == (3, 3 * nbytes + table_bytes(kind, handover))
    chain.release(0, 2)
    assert chain.advice(0) is None and chain.memory()[0] == 1
    if handover == "advice":                           # the host copy went with the release: nothing to upload again
        with pytest.raises(VdfError) as e:
            chain.materialize(ctx, 0, 1)
        assert e.value.code == VDF_ERR_BAD_ARG and "step 0 was released" in str(e.value)
    else:                                              # checkpoints stay: the step is walked again
        assert chain.materialize(ctx, 0, 1) == [0]
        assert dev_read(ctx, chain.advice(0), nbytes).tobytes() == advice_of(kind, field, L, 0).tobytes()
    assert dev_read(ctx, chain.advice(2), nbytes).tobytes() == advice_of(kind, field, L, 2).tobytes()
    chain.free()


# ---- 4. beyond the chain -------------------------------------------------------------------------------------------------------------
def test_a_step_not_yet_pushed_is_beyond_the_chain(ctx):
    kind, field = "rescue", FIELD_FQ
    pp, c, chain, proof = params(ctx, kind, field), circuit(kind, field), begin(kind, field, 1, "checkpoints"), None
    z0 = z_of(kind, field, 1, 0)
    for k in range(STEPS):
        with pytest.raises(VdfError) as e:
            NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
        assert e.value.code == VDF_ERR_BAD_ARG and "step %d is beyond the chain" % k in str(e.value)
        push(chain, kind, field, 1, "checkpoints", k)
        chain.materialize(ctx, k, 1, wait=False)
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)       # the same proof object goes on
        chain.release(k, 1)
    assert proof.serialize() == reference(ctx, kind, field)
    proof.free(); chain.free()


# ---- 5. the whole-chain prover -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handover", ["checkpoints", "advice"])
def test_the_whole_chain_prover_over_a_chain_pushed_completely(ctx, handover):
    kind, field = "rescue", FIELD_FQ
    pp, chain = params(ctx, kind, field), begin(kind, field, 1, handover)
    for g in range(STEPS):
        push(chain, kind, field, 1, handover, g)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(kind, field), chain, z_of(kind, field, 1, 0), window_steps=2, check_steps=True)
    assert proof.num_steps() == STEPS and proof.serialize() == reference(ctx, kind, field)
    assert chain.memory() == (0, table_bytes(kind, handover))
    proof.free(); chain.free()


# ---- 6. custom_ahead over a chain grown one step ahead of the prover -------------------------------------------------------------------
@pytest.mark.parametrize("handover", ["checkpoints", "advice"])
def test_the_lookahead_rides_over_the_step_pushed_ahead(ctx, handover):
    kind, field = "rescue", FIELD_FQ
    pp, c, chain, proof = params(ctx, kind, field, custom_ahead=2), circuit(kind, field), begin(kind, field, 1, handover), None
    z0 = z_of(kind, field, 1, 0)
    push(chain, kind, field, 1, handover, 0)
    chain.materialize(ctx, 0, 1, wait=True)
    for k in range(STEPS):
        if k + 1 < STEPS:                              # step k + 1 is there, and resolved, before step k is proved
            push(chain, kind, field, 1, handover, k + 1)
            chain.materialize(ctx, k + 1, 1, wait=True)
        proof = NovaVDFProof.prove_step_custom_chain(pp, proof, c, chain, k, z0)
        chain.release(k, 1)
    hits, misses, skipped = proof.ahead_stats()
    assert proof.serialize() == reference(ctx, kind, field)
    assert hits + misses + skipped == STEPS - 1 and hits >= 1 and misses == 0
    proof.free(); chain.free()


# ---- 7. eval_and_prove_custom --------------------------------------------------------------------------------------------------------
def stream(ctx, kind, field, lanes, every, c=None, **tune):
    forward, rebuild, direction = tapes(kind, field)
    inv, jb = inv_and_j_base(kind, field, lanes)
    walk = rebuild if direction == CHAIN_DESCENDING else None
    return NovaVDFProof.eval_and_prove_custom(params(ctx, kind, field, lanes, **tune), c or circuit(kind, field, lanes), forward, inv, T,
                                              initial_of(kind, field, lanes), STEPS, z_of(kind, field, lanes, 0), every=every, walk_tape=walk,
                                              walk_inv=inv if walk is not None else None, lanes=lanes, j_base=jb)


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("kind,every", [("rescue", 0), ("rescue", EVERY), ("minroot", EVERY)],
                         ids=["whole traces", "checkpoints ascending", "checkpoints by the MinRoot walk tape"])
def test_eval_and_prove_custom(ctx, kind, every, lanes):
    field = FIELD_FQ
    pp = params(ctx, kind, field, lanes)
    proof, final, stats = stream(ctx, kind, field, lanes, every)
    assert proof.num_steps() == STEPS and proof.serialize() == reference(ctx, kind, field, lanes)
    assert final.tobytes() == final_of(kind, field, lanes).tobytes()
    assert stats["steps"] == STEPS and stats["max_backlog"] >= 1 and stats["eval_ms"] > 0 and stats["after_eval_ms"] > 0
    assert proof.verify(pp, STEPS, z_of(kind, field, lanes, 0), z_of(kind, field, lanes, STEPS)) is True
    proof.free()


def test_eval_and_prove_custom_under_the_lookahead(ctx):
    proof, _, _ = stream(ctx, "rescue", FIELD_FQ, 1, EVERY, custom_ahead=2)
    hits, misses, skipped = proof.ahead_stats()
    assert proof.serialize() == reference(ctx, "rescue") and hits + misses + skipped == STEPS - 1 and misses == 0
    proof.free()


class FailsAtStepTwo(fs.Rescue):
    """the Rescue circuit whose third proved step raises"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.proved = 0

    def synthesize(self, cs, z):
        if cs.is_witness and not cs.is_probe:
            self.proved += 1
            if self.proved == 3:
                raise RuntimeError("the circuit gives up at step 2")
        return super().synthesize(cs, z)


@pytest.mark.parametrize("every", [0, EVERY])
def test_a_synthesize_that_fails_ends_the_call_and_the_next_call_works(ctx, every):
    kind, field = "rescue", FIELD_FQ
    with pytest.raises(RuntimeError, match="gives up at step 2"):
        stream(ctx, kind, field, 1, every, c=FailsAtStepTwo(T, table(field)[1], field))
    proof, final, stats = stream(ctx, kind, field, 1, every)          # the evaluators were joined, nothing was left half-pushed
    assert proof.serialize() == reference(ctx, kind, field) and stats["steps"] == STEPS
    assert final.tobytes() == final_of(kind, field, 1).tobytes()
    proof.free()


# ---- 8. the C example ----------------------------------------------------------------------------------------------------------------
def test_the_c_example_proves_a_chain_while_it_is_evaluated(ctx):
    exe = os.path.join(ROOT, "examples", "prove_custom_stream")
    assert os.path.exists(exe), "examples/prove_custom_stream is built by vdf_amd/csrc/Makefile (all)"
    src = open(exe + ".c").read()
    # no inverse tape anywhere in the file
    assert "vdf_nova_walk_body_record" not in src and "vdf_round_tape_walk" not in src and "_from_checkpoints" not in src
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(T), str(EVERY), str(STEPS), str(ROWS), str(0x51DE)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true" and lines["stream"].startswith("%d steps" % STEPS)
    kind, field = "rescue", FIELD_FQ
    pp = params(ctx, kind, field)
    assert int(lines["digest"], 16) == pp.digest()
    # the same chain proved through from_checkpoints_forward in this process
    cps = np.concatenate([c.reshape(-1, 16)[::EVERY].reshape(-1, 4) for c in chains_of(kind, field, 1)])
    chain = CustomChain.from_checkpoints(field, tapes(kind, field)[0], None, T, EVERY, STEPS, cps, forward=True)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(kind, field), chain, z_of(kind, field, 1, 0), window_steps=2)
    assert lines["running proof sha256"] == hashlib.sha256(proof.serialize()).hexdigest()
    snark = proof.compress(pp)
    assert lines["compressed proof sha256"] == hashlib.sha256(snark.serialize()).hexdigest()
    snark.free(); proof.free(); chain.free()
