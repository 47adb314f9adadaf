"""GPU: the forward MinRoot step circuit in lanes (include/vdf_nova.h VDF_CIRCUIT_MINROOT_FORWARD_LANES) -- L chains advanced
by one step circuit and attested by ONE proof.  The two kernels (vdf_minroot_forward_segment_lanes,
vdf_nifs_cross_term_minroot_forward_lanes) against their single-lane counterparts and the generic sparse kernel; whole proofs
against oracle/nova.py through its `primary=` seam over tests/lanes_spec.py; chains that grow in lanes, checkpoints out of
vdf_minroot_eval_batch, the wire, the batch calls and the plain-C client.  Every comparison is of bytes."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import vdf_amd
from oracle import nova as nv, pasta as o
from lanes_spec import LanesForwardCircuit, chains, flat, oracle_pp
from test_gpu_nova import aff_ints, check_instance, _canon
from util import dev, forward_segment_expected, host, limbs, mont, unmont, rand_limbs, states_array
from vdf_amd._lib import lib
from vdf_amd.hip import VdfError
from vdf_amd.minroot import EvalMode, PallasVDF, State, FIELD_FQ
from vdf_amd.nova import (CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_FORWARD, CIRCUIT_MINROOT_FORWARD_LANES, STENCIL_FORWARD, STENCIL_FORWARD_LANES,
                          GENS_KNOWN_DLOG, GENS_TRY_AND_INCREMENT, PP_NO_DIGIT_TABLES, INST_RUNNING_PRIMARY, INST_RUNNING_SECONDARY,
                          INST_FRESH_SECONDARY, INST_FRESH_PRIMARY_LAST, CompressedNovaVDFProof, ForwardCircuits, InverseMinRootCircuit,
                          LaneCircuits, NovaVDFProof, compress_batch, public_params, public_params_lanes, shape_digest_lanes,
                          shape_export_lanes, shape_stencil_lanes, verify_batch, verify_compressed_batch)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = EvalMode.LTRAddChainSequential
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


def zflat(states):
    return [e for s in states for e in (s.x, s.y, s.i)]


def lane_initials(L, seed, i0=None):
    """(States, the same as oracle ints): lane l starts at (rand(seed, l), 0, i0[l])"""
    i0 = i0 if i0 is not None else [7 * l for l in range(L)]
    ints = [(o.rand_fe(seed, l, o.Q), 0, i0[l]) for l in range(L)]
    return [State.from_ints(FIELD_FQ, *v) for v in ints], ints


def host_lanes(t, n, inits):
    """states[k][l] and traces[k][l] of n steps of t rounds per lane by the host evaluator"""
    vdf = PallasVDF.new_with_mode(FAST)
    states, traces = [list(inits)], []
    for _ in range(n):
        res = [vdf.eval_with_trace(s, t) for s in states[-1]]
        states.append([r[0] for r in res])
        traces.append([r[1] for r in res])
    return states, traces


def device_checkpoints(ctx, inits, rounds, every):
    """vdf_minroot_eval_batch: uint64[L, rounds / every + 1, 12], lane l's states every `every` rounds"""
    L, per = len(inits), rounds // every + 1
    out = np.zeros((L * per, 12), dtype="<u8")
    ctx.minroot_eval_batch(FIELD_FQ, states_array(inits), L, rounds, out, every=every)
    ctx.sync()
    return out.reshape(L, per, 12)


def as_states(rows):
    return [State(r[0:4].tobytes(), r[4:8].tobytes(), r[8:12].tobytes()) for r in rows]


def traces_chain(t, inits, traces):
    z0, lc = LaneCircuits.begin(t, inits)
    for step in traces:
        lc.push_traces(step)
    return z0, lc


# ---- the kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("L,t", [(1, 1), (2, 1), (3, 5), (3, 21), (2, 22), (4, 257)])
def test_segment_in_lanes_equals_the_single_lane_calls(ctx, cref, field, L, t):
    """vdf_minroot_forward_segment_lanes against the C restatement (its evaluator's traces, its field multiplication twice, the
    end counters: what test_gpu_forward.py::test_forward_segment expects of one lane) and against L calls of
    vdf_minroot_forward_segment -- one launch of L lanes against L launches of one, which is the lanes' offsets and strides --
    byte for byte, with the lanes' traces t + 1 and t + 3 entries apart (3t + 1 = 64 at t = 21 and 67 at t = 22: lanes end on and
    across a wavefront); the words around the output survive."""
    m = o.modulus(field)
    per, pad = 3 * t + 1, 7
    trs, ends, expected = [], cref.fe_array(L), []
    for l in range(L):
        st = mont([o.rand_fe(900 + t, 2 * l, m), o.rand_fe(900 + t, 2 * l + 1, m), 9 + 1000 * l], m)
        tr, i_end, words = forward_segment_expected(cref, field, st, t)
        trs.append(tr)
        ends[l] = i_end[0]
        expected.append(words)
    expected = np.concatenate(expected)
    want = []
    for l in range(L):
        one = dev(np.full((per, 4), FILL, dtype="<u8"))
        ctx.minroot_forward_segment(field, dev(trs[l]), t, ends[l:l + 1].copy(), one)
        want.append(one)
    ctx.sync()
    want = np.concatenate([host(w) for w in want])
    assert np.array_equal(want, expected)
    for stride in (t + 1, t + 3):
        buf = np.full((L * stride * 2, 4), FILL, dtype="<u8")
        for l in range(L):
            buf[2 * l * stride:2 * l * stride + 2 * (t + 1)] = trs[l]
        out = dev(np.full((L * per + 2 * pad, 4), FILL, dtype="<u8"))
        ctx.minroot_forward_segment_lanes(field, dev(buf), stride, t, L, ends.copy(), out[pad:])
        ctx.sync()
        got = host(out)
        assert np.array_equal(got[pad:pad + L * per], expected), stride
        assert np.array_equal(got[pad:pad + L * per], want), stride
        assert np.all(got[:pad] == FILL) and np.all(got[pad + L * per:] == FILL), stride
    d_tr, out = dev(buf), dev(np.zeros((L * per, 4), dtype="<u8"))
    with pytest.raises(VdfError):
        ctx.minroot_forward_segment_lanes(field, d_tr, t, t, L, ends.copy(), out)              # the lanes' traces would overlap
    with pytest.raises(VdfError):
        ctx.minroot_forward_segment_lanes(field, d_tr, t + 3, t, 0, ends.copy(), out)
    with pytest.raises(VdfError):
        ctx.minroot_forward_segment_lanes(field, d_tr, t + 3, t, 17, np.zeros((17, 4), dtype="<u8"), out)
    with pytest.raises(VdfError):
        ctx.minroot_forward_segment_lanes(field, d_tr, t + 3, t, L, dev(ends), out)            # i_end is a host operand
    with pytest.raises(VdfError):
        ctx.minroot_forward_segment_lanes(field, buf, t + 3, t, L, ends.copy(), out)           # the trace is a device operand


@pytest.mark.parametrize("L,t", [(1, 1), (1, 2), (1, 22), (2, 1), (2, 2), (3, 3), (3, 21), (2, 22), (4, 64)])
def test_stencil_in_lanes_equals_the_sparse_kernel(ctx, L, t):
    """vdf_nifs_cross_term_minroot_forward_lanes against vdf_nifs_cross_term_rows(.., VDF_ROWS_INSIDE) over the shape the
    parameters themselves are made of (its digest is the oracle's: tests/test_lanes_host.py): the same random z2 (constant
    column random, then ONE), random running vectors; A z2, B z2, C z2 and T equal, every row outside the range untouched.
    L = 1 is the single chain through the same entry point (stencil code 5): at t = 1, 2 its j = 0, 1 rows, which read z_in, are
    most or all of it, and at t = 22 it ends across a wavefront."""
    field, m = o.FIELD_FQ, o.Q
    code, row0, nr, S = shape_stencil_lanes(t, L)
    assert code == (STENCIL_FORWARD if L == 1 else STENCIL_FORWARD_LANES) and nr == L * (3 * t + 1)
    mats = shape_export_lanes(t, L, 0)
    nc, nvars = shape_digest_lanes(t, L, 1)[1][0][:2]
    ncols = nvars + 3                                               # z = (W, u, X)
    assert S + nr <= nvars and row0 + nr <= nc and all(int(mt[1].max()) < ncols for mt in mats)
    shape = ctx.shape_create(field, nc, ncols, mats)
    rng = np.random.default_rng(7 * t + L)
    abc1 = [dev(rand_limbs(rng, nc)) for _ in range(3)]
    u1 = rand_limbs(rng, 1)
    for unit in (False, True):
        z2 = rand_limbs(rng, ncols)
        if unit:
            z2[nvars] = limbs([o.to_mont(1, m)])[0]
        else:
            assert unmont(z2[nvars:nvars + 1], m) != [1]
        want = [dev(np.full((nc, 4), FILL, dtype="<u8")) for _ in range(4)]
        got = [dev(np.full((nc, 4), FILL, dtype="<u8")) for _ in range(4)]
        ctx.nifs_cross_term_rows(shape, row0, nr, 1, dev(z2), *abc1, u1, *want)
        ctx.nifs_cross_term_minroot_forward_lanes(field, t, L, S, nvars, row0, dev(z2), *abc1, u1, *got)
        ctx.sync()
        for k, (g, w) in enumerate(zip(got, want)):
            g, w = host(g), host(w)
            assert np.array_equal(g[row0:row0 + nr], w[row0:row0 + nr]), (unit, "ABCT"[k])
            assert np.all(g[:row0] == FILL) and np.all(g[row0 + nr:] == FILL), (unit, "ABCT"[k])
    with pytest.raises(VdfError):
        ctx.nifs_cross_term_minroot_forward_lanes(field, t, L, S, S + nr - 1, row0, dev(z2), *abc1, u1, *got)   # the constant inside the rounds
    with pytest.raises(VdfError):
        ctx.nifs_cross_term_minroot_forward_lanes(field, t, L, 3 * L - 1, nvars, row0, dev(z2), *abc1, u1, *got)   # no room for the inputs
    with pytest.raises(VdfError):
        ctx.nifs_cross_term_minroot_forward_lanes(field, t, 17, S, nvars, row0, dev(z2), *abc1, u1, *got)
    with pytest.raises(VdfError):
        ctx.nifs_cross_term_minroot_forward_lanes(field, t, L, S, nvars, row0, dev(z2), *abc1, dev(u1), *got)   # u1 is a host operand
    shape.free()


# ---- proofs against the oracle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("L,t,n", [(2, 3, 3), (3, 5, 2)])
def test_prove_steps_replayed_by_the_oracle(ctx, L, t, n):
    """Every step's fresh and running instances with their witnesses, both cross-term commitments and both challenges equal
    oracle.nova.prove_step's over the specification circuit; verify(z0 = the initial states, zi = the final ones) passes."""
    inits, ints = lane_initials(L, 70 + L, i0=[1 + 50 * l for l in range(L)])
    states, traces = host_lanes(t, n, inits)
    pp = public_params_lanes(ctx, t, L)
    assert pp.lanes() == L and pp.circuit_kind == CIRCUIT_MINROOT_FORWARD_LANES and pp.segment()[1] == L * (3 * t + 1)
    z0, lc = traces_chain(t, inits, traces)
    com = nv.CCommit()
    opp = oracle_pp(t, L, com)
    assert pp.digest() == opp.params
    for side in (0, 1):
        sz, sh = pp.sizes(side), opp.shapes[side]
        assert (sz["num_cons"], sz["num_vars"], sz["num_io"], sz["nnz"]) == (sh.num_cons, sh.num_vars, 2, len(sh.A) + len(sh.B) + len(sh.C))
    ost = chains([o.State(*v) for v in ints], t, n)
    assert [[s.to_ints(FIELD_FQ) for s in row] for row in states] == [[(s.x, s.y, s.i) for s in row] for row in ost]
    z0i = flat(ost[0])
    proof, want = None, None
    for k in range(n):
        proof = NovaVDFProof.prove_step(pp, proof, lc, k, z0)
        want = nv.prove_step(opp, want, LanesForwardCircuit(t, ost[k], ost[k + 1]), z0i)
        tr, ls = want.trace[-1], proof.last_step()
        assert aff_ints(ls["comm_W1"], 0) == tuple(tr["l1"].comm_W) and unmont(ls["X1"], o.Q) == tr["l1"].X
        if k:
            assert aff_ints(ls["comm_T1"], 0) == tuple(tr["T1"]) and aff_ints(ls["comm_T2"], 1) == tuple(tr["T2"])
            assert (ls["r1"], ls["r2"]) == (tr["r1"], tr["r2"])
        check_instance(proof, INST_RUNNING_PRIMARY, 0, want.r[0])
        check_instance(proof, INST_RUNNING_SECONDARY, 1, want.r[1])
        check_instance(proof, INST_FRESH_SECONDARY, 1, want.l2)
        zp, zs = proof.zi()
        assert unmont(zp, o.Q) == want.zi[0] == flat(ost[k + 1]) and unmont(zs, o.P) == want.zi[1]
    zi = zflat(states[n])
    assert z0 == zflat(states[0])
    assert proof.verify(pp, n, z0, zi) is True
    assert proof.verify(pp, n + 1, z0, zi) is False and proof.verify(pp, n, zi, z0) is False
    proof.free(); lc.free(); pp.free()


def test_one_lane_is_the_forward_circuit(ctx):
    """lanes = 1: the parameters are those of VDF_CIRCUIT_MINROOT_FORWARD, a lanes chain of one lane is a forward chain, and the
    running and compressed wire bytes equal those of a kind-3 proof of the same chain."""
    t, n = 16, 3
    inits, _ = lane_initials(1, 5)
    states, traces = host_lanes(t, n, inits)
    pp1 = public_params_lanes(ctx, t, 1)
    pp3 = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)
    assert pp1.circuit_kind == CIRCUIT_MINROOT_FORWARD and pp1.lanes() == 1 == pp3.lanes() and pp1.digest() == pp3.digest()
    assert pp1.stencil() == pp3.stencil() and pp1.segment() == pp3.segment()
    z0, lc = traces_chain(t, inits, traces)
    z03, fc = ForwardCircuits.begin(t, inits[0])
    for k in range(n):
        fc.push_trace(traces[k][0])
    a = NovaVDFProof.prove_recursively(pp1, lc, t, z0)
    b = NovaVDFProof.prove_recursively(pp3, fc, t, z03)
    assert z0 == z03 and a.serialize() == b.serialize()
    ca, cb = a.compress(pp1), b.compress(pp3)
    assert ca.serialize() == cb.serialize() and ca.verify(pp1, n, z0, zflat(states[n]))
    for h in (ca, cb, a, b, lc, fc, pp1, pp3):
        h.free()
    for lanes in (0, 17):
        with pytest.raises(VdfError):
            public_params_lanes(ctx, t, lanes)


# ---- one proof, several ways --------------------------------------------------------------------------------------

def test_one_proof_several_ways(ctx):
    """L = 3, t = 16, 4 steps, the chains evaluated by vdf_minroot_eval_batch on the device: (a) every step pushed as traces,
    then prove_recursively; (b) push one, prove one, release one; (c) checkpoints straight out of the batch with every = t and
    t / 4, materialised; (d) the same never materialised, in windows of 2; (e) stencil = 0 -- one set of wire bytes."""
    L, t, n = 3, 16, 4
    inits, _ = lane_initials(L, 19, i0=[2, 0, 1000])
    states, traces = host_lanes(t, n, inits)
    pp = public_params_lanes(ctx, t, L)
    tn = pp.tuning()
    if tn["stencil"] == 1 and tn["early_rows"] != 0:
        assert pp.stencil() == STENCIL_FORWARD_LANES and pp.early_rows()[1] == L * (3 * t + 1) == pp.segment()[1]
    zi = zflat(states[n])
    z0, lc = traces_chain(t, inits, traces)
    a = NovaVDFProof.prove_recursively(pp, lc, t, z0)
    assert a.verify(pp, n, z0, zi)
    wire = a.serialize()
    # (b)
    z0b, lb = LaneCircuits.begin(t, inits)
    b = None
    for k in range(n):
        lb.push_traces(traces[k])
        b = NovaVDFProof.prove_step(pp, b, lb, k, z0b)
        lb.release(k, 1)
        assert lb.host_bytes() == 0
    assert z0b == z0 and b.serialize() == wire
    # (c), (d): the device's checkpoints, fed in unchanged
    for every in (t, t // 4):
        cps = device_checkpoints(ctx, inits, t * n, every)
        per, stride = t // every, t * n // every + 1
        assert [as_states(cps[:, k * per])for k in range(n + 1)] == states
        z0c, lcp = LaneCircuits.begin(t, inits)
        for k in range(n):
            lcp.push_checkpoints(every, cps.reshape(-1, 12)[k * per:], lane_stride=stride)
        assert len(lcp) == n and lcp.lane_states(n - 1, 2) == (states[n][2], states[n - 1][2]) and lcp.memory() == (0, 0)
        assert lcp.host_bytes() == n * L * (per + 1) * 96
        with pytest.raises(VdfError):
            NovaVDFProof.prove_step(pp, None, lcp, 0, z0c)             # no trace yet
        assert lcp.materialize(ctx) == [0] * n and lcp.memory() == (n, n * L * (t + 1) * 64)
        # a rebuilt trace is the evaluator's: the lanes' traces back to back
        got = np.zeros(L * (t + 1) * 8, dtype="<u8")
        assert lib.vdf_dev_memcpy(ctx.handle, got.ctypes.data, lcp.trace_ptr(2), got.nbytes) == 0
        assert np.array_equal(got.reshape(L, -1, 4), np.stack([np.asarray(x).reshape(-1, 4) for x in traces[2]]))
        c = NovaVDFProof.prove_recursively(pp, lcp, t, z0c)
        assert c.serialize() == wire
        lcp.release()
        assert lcp.memory() == (0, 0)
        d = NovaVDFProof.prove_recursively(pp, lcp, t, z0c, window_steps=2)
        assert d.serialize() == wire and lcp.memory() == (0, 0)
        c.free(); d.free(); lcp.free()
    # (e)
    pp0 = public_params_lanes(ctx, t, L, stencil=0)
    assert pp0.stencil() == 0 and pp0.early_rows() == pp.early_rows() and pp0.digest() == pp.digest()
    e = NovaVDFProof.prove_recursively(pp0, lc, t, z0)
    assert e.serialize() == wire
    for h in (a, b, e, lb, lc, pp0, pp):
        h.free()


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    """A checkpoint changed in lane 2 of step 1: materialize flags exactly that step.  verify refuses a z0 changed in lane 1
    and a zi with two lanes swapped.  Parameters and circuits of different kinds or lane counts do not mix."""
    L, t, n = 3, 16, 3
    inits, _ = lane_initials(L, 23)
    states, traces = host_lanes(t, n, inits)
    every, per = 4, 4
    vdf = PallasVDF.new_with_mode(FAST)
    cps = [vdf.eval_checkpoints(s, t * n, every) for s in inits]
    z0t, lt = LaneCircuits.begin(t, inits)
    for k in range(n):
        part = [list(c[k * per:(k + 1) * per + 1]) for c in cps]
        if k == 1:
            x = bytearray(part[2][2].x)
            x[9] ^= 0x10
            part[2][2] = State(bytes(x), part[2][2].y, part[2][2].i)
        lt.push_checkpoints(every, part)
    with pytest.raises(VdfError) as err:
        lt.materialize(ctx)
    assert lt.last_bad == [0, 1, 0] and "circuit 1" in str(err.value)
    lt.free()
    pp = public_params_lanes(ctx, t, L)
    z0, lc = traces_chain(t, inits, traces)
    proof = NovaVDFProof.prove_recursively(pp, lc, t, z0)
    zi = zflat(states[n])
    assert proof.verify(pp, n, z0, zi) is True
    bad = list(z0)
    bad[3] = inits[0].x                                               # lane 1 claims lane 0's start
    assert proof.verify(pp, n, bad, zi) is False
    assert proof.verify(pp, n, z0, zi[3:6] + zi[0:3] + zi[6:]) is False
    assert proof.verify(pp, n, z0, zi[0:3] + zi[6:9] + zi[3:6]) is False
    # kinds and lane counts
    pp2 = public_params_lanes(ctx, t, 2)
    pp3 = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)
    ppb = public_params(ctx, t, CIRCUIT_MINROOT_BOUND)
    z02, l2 = traces_chain(t, inits[:2], [s[:2] for s in traces])
    z03, fc = ForwardCircuits.begin(t, inits[0])
    fc.push_trace(traces[0][0])
    z0b, inv = InverseMinRootCircuit.eval_and_make_circuits(vdf, t, 1, inits[0])
    for p, c, z in ((pp, l2, z02), (pp2, lc, z0), (pp3, lc, z0), (pp, fc, z03), (ppb, lc, z0), (pp, inv, z0b)):
        with pytest.raises(VdfError):
            NovaVDFProof.prove_step(p, None, c, 0, list(z) + [bytes(32)] * (9 - len(z)))      # (as many elements as the widest arity)
    with pytest.raises(VdfError):
        NovaVDFProof.prove_step(pp, None, lc, 1, z0)                   # step 1 first: z0 is not its input
    with pytest.raises(VdfError):
        NovaVDFProof.eval_and_prove(pp, vdf, inits[0], 2)              # its evaluator is one chain
    # fold_fused has no lanes kernel: the parameters are made and the proof is the unfused one
    ppf = public_params_lanes(ctx, t, L, fold_fused=1)
    f = NovaVDFProof.prove_recursively(ppf, lc, t, z0)
    assert f.serialize() == proof.serialize()
    for h in (f, proof, lc, l2, fc, inv, pp, pp2, pp3, ppb, ppf):
        h.free()


# ---- the wire and the batch calls -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_lanes():
    with open(os.path.join(ROOT, "tests", "golden", "lanes.json")) as f:
        return json.load(f)


def test_wire_and_batches(ctx, golden_lanes):
    """compress -> wire -> deserialize under a second context -> verify_compressed; the SHA-256 of both wire encodings at
    L = 2, t = 3, 3 steps is the oracle-derived one of tests/golden/lanes.json; the proof passes the batch verifiers beside a
    second lanes proof, and a tampered copy fails alone."""
    g = golden_lanes["wire_L2_t3_n3"]
    L, t, n = g["lanes"], g["t"], g["steps"]
    inits, _ = lane_initials(L, g["seed"], i0=g["i0"])
    states, traces = host_lanes(t, n, inits)
    pp = public_params_lanes(ctx, t, L)
    assert pp.digest() == int(g["params"], 16)
    z0, lc = traces_chain(t, inits, traces)
    zi = zflat(states[n])
    proof = NovaVDFProof.prove_recursively(pp, lc, t, z0)
    running = proof.serialize()
    assert len(running) == g["running_proof_len"] and hashlib.sha256(running).hexdigest() == g["running_proof_sha256"]
    snark = proof.compress(pp)
    wire = snark.serialize()
    assert wire[:8] == b"VDFSNK03" and len(wire) == g["compressed_proof_len"]
    assert hashlib.sha256(wire).hexdigest() == g["compressed_proof_sha256"]
    swapped = zi[3:6] + zi[0:3]
    assert snark.verify(pp, n, z0, zi) and not snark.verify(pp, n, z0, swapped) and not snark.verify(pp, n + 1, z0, zi)
    ctx2 = vdf_amd.Context(0)
    pp2 = public_params_lanes(ctx2, t, L)
    again = CompressedNovaVDFProof.deserialize(pp2, wire)
    assert again.verify(pp2, n, z0, zi) and again.serialize() == wire
    resumed = NovaVDFProof.deserialize(pp2, running)
    assert resumed.verify(pp2, n, z0, zi) and resumed.serialize() == running
    ppf = public_params(ctx2, t, CIRCUIT_MINROOT_FORWARD)               # other parameters refuse the bytes
    with pytest.raises(VdfError):
        CompressedNovaVDFProof.deserialize(ppf, wire)
    for h in (again, resumed, pp2, ppf):
        h.free()
    ctx2.close()
    # a second lanes proof under the same parameters, one step longer, for the batches
    inits2 = [states[1][1], states[2][0]]
    states2, traces2 = host_lanes(t, 4, inits2)
    z0_2, l2 = traces_chain(t, inits2, traces2)
    p2 = NovaVDFProof.prove_recursively(pp, l2, t, z0_2)
    zi_2 = zflat(states2[4])
    assert verify_batch(pp, [(proof, n, z0, zi), (p2, 4, z0_2, zi_2), (proof, n, z0, swapped), (p2, 3, z0_2, zi_2)]) == [True, True, False, False]
    snarks = compress_batch(pp, [proof, p2])
    assert snarks[0].serialize() == wire and snarks[1].serialize() == p2.compress(pp).serialize()
    tampered = bytearray(wire)
    tampered[-5] ^= 1
    try:
        bad = CompressedNovaVDFProof.deserialize(pp, bytes(tampered))
    except VdfError:
        bad = None                                                      # not canonical any more: refused at the door
    items = [(snarks[0], n, z0, zi), (snarks[1], 4, z0_2, zi_2), (snarks[1], 4, z0, zi_2)] + ([(bad, n, z0, zi)] if bad else [])
    assert verify_compressed_batch(pp, items) == [True, True, False] + ([False] if bad else [])
    for h in snarks + [snark, proof, p2, lc, l2, pp] + ([bad] if bad else []):
        h.free()


# ---- at size ----------------------------------------------------------------------------------------------------------

def test_at_size_eight_lanes_of_8192(ctx, cref):
    """L = 8, t = 8,192 (L t = 2^16), 2 steps, generators of known discrete logarithm, no digit tables: stencil code 6; the
    fresh and the folded commitments pass the discrete-log identity; verify is true; the proof's bytes equal those made with
    stencil = 0 (the generic sparse kernel)."""
    L, t, n = 8, 8192, 2
    fld = o.FIELD_FQ
    inits, _ = lane_initials(L, 3, i0=[1 + l for l in range(L)])
    every = t // 4
    cps = device_checkpoints(ctx, inits, t * n, every)
    per, stride = t // every, t * n // every + 1
    pp = public_params_lanes(ctx, t, L, GENS_KNOWN_DLOG, flags=PP_NO_DIGIT_TABLES)
    tn = pp.tuning()
    if not (tn["stencil"] == 1 and tn["early_rows"] != 0):
        pytest.skip("the environment overrides the defaults under test (tools/gpu_env_matrix.sh)")
    assert pp.stencil() == STENCIL_FORWARD_LANES == 6 and pp.early_rows()[1] == L * (3 * t + 1) == pp.segment()[1]
    nvar = pp.sizes(0)["num_vars"]
    z0, lc = LaneCircuits.begin(t, inits)
    for k in range(n):
        lc.push_checkpoints(every, cps.reshape(-1, 12)[k * per:], lane_stride=stride)
    assert lc.materialize(ctx) == [0] * n
    proof = None
    for k in range(n):
        proof = NovaVDFProof.prove_step(pp, proof, lc, k, z0)
    ls = proof.last_step()
    z2, _ = proof.witness(INST_FRESH_PRIMARY_LAST)
    z_new, E_new = proof.witness(INST_RUNNING_PRIMARY)
    inst_new = proof.instance(INST_RUNNING_PRIMARY)
    seg_b, seg_n = pp.segment()
    mid = as_states(cps[:, per])                                        # z_in of the last step: every lane's state after step 0
    assert np.array_equal(z2[seg_b - 3 * L:seg_b], np.frombuffer(b"".join(zflat(mid)), dtype="<u8").reshape(3 * L, 4))
    ends = np.stack([cps[l, 2 * per, 8:12] for l in range(L)])          # final_i of every lane
    assert np.array_equal(z2[seg_b + 3 * t:seg_b + seg_n:3 * t + 1], ends)
    dl = lambda vec: o.msm_by_dlog_limbs(_canon(cref, fld, np.ascontiguousarray(vec)), o.CURVE_PALLAS, nv.GENS_SEED) or (0, 0)
    assert aff_ints(ls["comm_W1"], 0) == dl(z2[:nvar])
    assert aff_ints(inst_new["comm_W"], 0) == dl(z_new[:nvar]) and aff_ints(inst_new["comm_E"], 0) == dl(E_new)
    zi = zflat(as_states(cps[:, 2 * per]))
    assert proof.verify(pp, n, z0, zi) is True
    wire = proof.serialize()
    proof.free()
    pp0 = public_params_lanes(ctx, t, L, GENS_KNOWN_DLOG, flags=PP_NO_DIGIT_TABLES, stencil=0)
    assert pp0.stencil() == 0 and pp0.early_rows() == pp.early_rows() and pp0.digest() == pp.digest()
    b = NovaVDFProof.prove_recursively(pp0, lc, t, z0)
    assert b.serialize() == wire
    b.free(); pp0.free(); lc.free(); pp.free()


# ---- the plain-C client ----------------------------------------------------------------------------------------

def test_prove_lanes_client(ctx, tmp_path):
    """examples/prove_lanes (plain C over the two ABIs) as a fresh child process at L = 3, t = 64, 2 steps: exit 0, every
    verification as expected, and the compressed proof it writes is byte for byte the Python host's for the same chains."""
    exe = os.path.join(ROOT, "examples", "prove_lanes")
    assert os.path.exists(exe), "examples/prove_lanes is built by vdf_amd/csrc/Makefile (all)"
    L, t, n, x0 = 3, 64, 2, 1000
    out_path = str(tmp_path / "wire.bin")
    # a fresh child process (never an exec of this one)
    r = subprocess.run([exe, str(L), "6", str(n), str(x0), out_path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true" and lines["verify with two outputs swapped"] == "false"
    assert "stencil code 6" in r.stdout and all(lines["lane %d" % l] == "check: ok" for l in range(L))
    inits = [State.from_ints(FIELD_FQ, x0 + l, 0, 7 * l) for l in range(L)]
    vdf = PallasVDF.new_with_mode(FAST)
    every, per = t // 4, 4
    cps = [vdf.eval_checkpoints(s, t * n, every) for s in inits]
    pp = public_params_lanes(ctx, t, L)
    z0, lc = LaneCircuits.begin(t, inits)
    for k in range(n):
        lc.push_checkpoints(every, [c[k * per:(k + 1) * per + 1] for c in cps])
    proof = NovaVDFProof.prove_recursively(pp, lc, t, z0)
    snark = proof.compress(pp)
    assert open(out_path, "rb").read() == snark.serialize()
    for h in (snark, proof, lc, pp):
        h.free()
