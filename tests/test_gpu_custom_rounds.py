"""GPU: repeated rounds of a custom step circuit run on the device (include/vdf_nova.h vdf_cs_repeat, include/vdf_hip.h
vdf_round_tape_run; the reference's extension point is its StepCircuit trait, src/nova/proof.rs:79-153).

a. the kernel alone against an existing kernel: the tape of the forward MinRoot round written through the seam equals the first
   3t variables of vdf_minroot_forward_segment byte for byte (sizes around the j < 2 region, the wavefront = workgroup edge of 64,
   the 256 edge of the kernel it is compared with, and many workgroups), in both fields;
b. a round that uses every op, on the device, against the host evaluator and a big-integer interpretation;
c. proofs made three ways -- repeat with device advice, repeat with host advice, the same circuit as a plain loop -- are the same
   bytes, verify, state the chain's states, compress to the same bytes; once in the Fp orientation;
d. inconsistent advice gives an unsatisfiable witness: prove_step succeeds, verify answers False, nothing faults;
e. the plain-C example, as a fresh child process."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import pasta as o
from util import dev, host, host_trace, ints, limbs
from rounds_spec import F, G, MOD, mont_rows
from vdf_amd.minroot import PallasVDF, State, VestaVDF
from vdf_amd.nova import (NovaVDFProof, public_params_custom, record_round_body, round_tape_eval, shape_digest_custom, FIELD_FP,
                          FIELD_FQ)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VDF = {FIELD_FQ: PallasVDF, FIELD_FP: VestaVDF}
T_MAX = 1024


@functools.lru_cache(maxsize=None)
def long_trace(field):
    """one chain of T_MAX rounds per field: a shorter step's trace is its head"""
    s0 = State.from_ints(field, 0x1234567 + field, 5, 3)
    _, tr = host_trace(VDF[field].new(), s0, T_MAX)
    return s0, tr


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("t", [1, 2, 5, 63, 64, 65, 257, 1024])
def test_a_forward_round_tape_equals_the_forward_segment_kernel(ctx, t, field):
    import torch
    s0, tr = long_trace(field)
    d_trace = dev(tr[:t + 1])
    tape = record_round_body(F(t, "repeat", field).body(), field)
    i_in = np.frombuffer(s0.i, dtype="<u8").reshape(1, 4).copy()
    i_end = limbs([o.to_mont((3 + t) % MOD[field], MOD[field])])
    want = torch.zeros((3 * t + 1, 4), dtype=torch.int64, device="cuda")
    got = torch.full((3 * t + 2, 4), -1, dtype=torch.int64, device="cuda")     # two guard elements behind the 3t variables
    ctx.minroot_forward_segment(field, d_trace, t, i_end, want)
    ctx.round_tape_run(field, tape, t, i_in, d_trace, got)
    ctx.sync()
    g, w = host(got), host(want)
    assert g[:3 * t].tobytes() == w[:3 * t].tobytes()
    assert (g[3 * t:] == np.uint64(2**64 - 1)).all()                             # nothing written past the last repetition


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("t", [65, 257])
def test_a_round_of_every_op_on_the_device(ctx, t, field):
    import torch
    m = MOD[field]
    rng = np.random.default_rng(t + field)
    k = 0x9E3779B97F4A7C15 % m
    adv = G.advice_for(0xABCDEF, k, t, m, rng, special=(0, 1, m - 1))
    tape = record_round_body(G(t, "repeat", field).body(), field)
    inv, adv_m = mont_rows([k], m), mont_rows(adv, m)
    got = torch.zeros((5 * t, 4), dtype=torch.int64, device="cuda")
    ctx.round_tape_run(field, tape, t, inv, dev(adv_m), got)
    ctx.sync()
    want = round_tape_eval(field, tape, t, inv, adv_m)
    assert host(got).tobytes() == want.tobytes()
    assert [o.from_mont(v, m) for v in ints(want)] == G.variables(adv, t, [k], m)


def test_the_launcher_refuses_a_malformed_tape(ctx):
    """every index is checked on the host before anything is launched"""
    import torch
    from vdf_amd.hip import VdfError
    _, tr = long_trace(FIELD_FQ)
    d_trace, out = dev(tr[:3]), torch.zeros((6, 4), dtype=torch.int64, device="cuda")
    i_in = mont_rows([3], o.Q)
    for field_name, value in (("a", 9), ("b", 2)):                  # an advice column / entry the tape does not have
        tape = record_round_body(F(2, "repeat").body())
        setattr(tape.ops[0], field_name, value)
        with pytest.raises(VdfError):
            ctx.round_tape_run(FIELD_FQ, tape, 2, i_in, d_trace, out)
    tape = record_round_body(F(2, "repeat").body())
    tape.ops[1].b = 64                                              # a variable beyond n_vars
    with pytest.raises(VdfError):
        ctx.round_tape_run(FIELD_FQ, tape, 2, i_in, d_trace, out)
    tape = record_round_body(F(2, "repeat").body())
    tape.c.n_slots = 25                                             # beyond the cap on LDS slots
    with pytest.raises(VdfError):
        ctx.round_tape_run(FIELD_FQ, tape, 2, i_in, d_trace, out)
    assert not host(out).any()


def chain(field, t, n):
    """n steps of t rounds: (z0 bytes, [trace uint64[t + 1, 8] per step], [State after each step])"""
    vdf = VDF[field].new()
    s = State.from_ints(field, 0x51DE + t, 0, 7)
    z0, traces, states = [s.x, s.y, s.i], [], []
    for _ in range(n):
        s, tr = host_trace(vdf, s, t)
        traces.append(tr)
        states.append(s)
    return z0, traces, states


def prove(ctx, field, t, mode, advice_of, traces, z0, bad=None):
    """the chain proved with circuit F in one of its forms; advice_of(trace) -> what the circuit is handed"""
    m = MOD[field]
    c = F(t, mode, field)
    pp = public_params_custom(ctx, c, field=field)
    proof, keep = None, []
    for k, tr in enumerate(traces):
        c.advice = advice_of(tr)
        c.advice_ints = [o.from_mont(v, m) for v in ints(tr)]
        keep.append(c.advice)
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
    ctx.sync()
    return pp, proof


def three_ways(ctx, field, t, n=3):
    z0, traces, states = chain(field, t, n)
    runs = [prove(ctx, field, t, "repeat", dev, traces, z0), prove(ctx, field, t, "repeat", lambda tr: tr, traces, z0),
            prove(ctx, field, t, "loop", lambda tr: None, traces, z0)]
    zi = [states[-1].x, states[-1].y, states[-1].i]
    assert runs[0][0].segment()[1] == 3 * t and runs[1][0].segment() == runs[0][0].segment() and runs[2][0].segment() == (0, 0)
    assert len({pp.digest() for pp, _ in runs}) == 1
    blobs = [proof.serialize() for _, proof in runs]
    assert blobs[0] == blobs[2] and blobs[1] == blobs[2]
    for pp, proof in runs:
        assert proof.verify(pp, n, z0, zi) is True
        assert proof.verify(pp, n, z0, [zi[1], zi[0], zi[2]]) is False
        assert b"".join(zi) == proof.zi()[0].tobytes()
    return runs, z0, zi


@pytest.mark.parametrize("t", [5, 65])
def test_three_ways_to_prove_the_same_chain_give_the_same_proof(ctx, t):
    runs, z0, zi = three_ways(ctx, FIELD_FQ, t)
    if t == 5:
        snarks = [proof.compress(pp) for pp, proof in runs]
        for (pp, _), s in zip(runs, snarks):
            assert s.verify(pp, 3, z0, zi) is True
        wires = [s.serialize() for s in snarks]
        assert wires[0] == wires[2] and wires[1] == wires[2]
    for pp, proof in runs:
        proof.free(); pp.free()


def test_three_ways_in_the_other_orientation(ctx):
    runs, _, _ = three_ways(ctx, FIELD_FP, 5)
    for pp, proof in runs:
        proof.free(); pp.free()


def test_inconsistent_advice_is_an_unsatisfiable_witness_not_a_fault(ctx):
    t, n = 65, 3
    z0, traces, states = chain(FIELD_FQ, t, n)
    zi = [states[-1].x, states[-1].y, states[-1].i]
    # one altered root in the middle of the second step's advice
    wrong = [tr.copy() for tr in traces]
    wrong[1][t // 2, 0] ^= np.uint64(1)
    pp, proof = prove(ctx, FIELD_FQ, t, "repeat", dev, wrong, z0)
    assert proof.zi()[0].tobytes() == b"".join(zi)                    # the last entries are intact: the statement is the chain's
    assert proof.verify(pp, n, z0, zi) is False
    proof.free()
    # the advice of another step: the carry does not continue the previous step's output
    c = F(t, "repeat", FIELD_FQ)
    proof, keep = None, []
    for tr in (traces[0], traces[2], traces[2]):
        c.advice = dev(tr)
        keep.append(c.advice)
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
    assert proof.verify(pp, n, z0, [bytes(r) for r in proof.zi()[0].view(np.uint8).reshape(3, 32)]) is False
    # and the intact chain under the same parameters still verifies
    proof.free()
    proof = None
    for tr in traces:
        c.advice = dev(tr)
        keep.append(c.advice)
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
    assert proof.verify(pp, n, z0, zi) is True
    proof.free(); pp.free()


def test_a_body_that_differs_from_the_parameters_is_refused(ctx):
    from vdf_amd.hip import VdfError
    t = 5
    z0, traces, _ = chain(FIELD_FQ, t, 1)
    pp = public_params_custom(ctx, F(t, "repeat"))
    other = F(t + 1, "repeat")
    other.advice = np.concatenate([traces[0], traces[0][:1]])
    with pytest.raises(VdfError):
        NovaVDFProof.prove_step_custom(pp, None, other, z0)
    plain = F(t, "loop")
    plain.advice_ints = [o.from_mont(v, o.Q) for v in ints(traces[0])]
    with pytest.raises(VdfError):
        NovaVDFProof.prove_step_custom(pp, None, plain, z0)
    pp.free()


def test_the_c_example_proves_through_the_seam():
    exe = os.path.join(ROOT, "examples", "prove_custom_rounds")
    assert os.path.exists(exe), "examples/prove_custom_rounds is built by vdf_amd/csrc/Makefile (all)"
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run([exe, "65", "3", "123"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify with z0 and zi swapped"] == "false"
    assert lines["rounds on the device"].startswith("%d variables" % (3 * 65))
    assert int(lines["digest"], 16) == shape_digest_custom(F(65, "repeat"))[0]
