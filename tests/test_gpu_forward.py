"""GPU: the forward MinRoot step circuit (include/vdf_nova.h VDF_CIRCUIT_MINROOT_FORWARD) -- a chain proved in the direction it
is evaluated, and while it is evaluated.  The two kernels (vdf_minroot_forward_segment, vdf_nifs_cross_term_minroot_forward)
against the specification circuit of tests/forward_spec.py and the generic sparse kernel; whole proofs against
oracle/nova.py through its `primary=` seam; growing chains, checkpoints, eval_and_prove, the wire and the batch calls.
Every comparison is of bytes."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import vdf_amd
from oracle import nova as nv, pasta as o
from forward_spec import ForwardMinRootCircuit, chain, oracle_pp
from test_gpu_nova import aff_ints, check_instance, _canon
from util import dev, forward_segment_expected, host, limbs, mont, unmont, rand_limbs
from vdf_amd._lib import lib
from vdf_amd.hip import VdfError
from vdf_amd.minroot import EvalMode, PallasVDF, State, FIELD_FQ
from vdf_amd.nova import (CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_FORWARD, STENCIL_FORWARD, GENS_KNOWN_DLOG, GENS_TRY_AND_INCREMENT,
                          INST_RUNNING_PRIMARY, INST_RUNNING_SECONDARY, INST_FRESH_SECONDARY, INST_FRESH_PRIMARY_LAST,
                          CompressedNovaVDFProof, ForwardCircuits, InverseMinRootCircuit, NovaVDFProof, compress_batch, nova_lib,
                          public_params, verify_batch, verify_compressed_batch)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = EvalMode.LTRAddChainSequential
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


def zvec(s):
    return [s.x, s.y, s.i]


def forward_chain(ctx, t, n, seed=42, i0=0, family=GENS_TRY_AND_INCREMENT, **tune):
    """(pp, z0, circuits with every trace pushed, [State] at the step boundaries, the traces, the initial state as ints)"""
    x = o.rand_fe(seed, 0, o.Q)
    initial = State.from_ints(FIELD_FQ, x, 0, i0)
    pp = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD, family, **tune)
    vdf = PallasVDF.new_with_mode(FAST)
    z0, fc = ForwardCircuits.begin(t, initial)
    states, traces = [initial], []
    for _ in range(n):
        s, tr = vdf.eval_with_trace(states[-1], t)
        states.append(s)
        traces.append(tr)
        fc.push_trace(tr)
    return pp, z0, fc, states, traces, (x, 0, i0)


# ---- the kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("t", [1, 5, 257, 65536])
def test_forward_segment(ctx, cref, field, t):
    """vdf_minroot_forward_segment: x_(j+1), its square and its fourth power per round from the forward trace, then final_i --
    against the C restatement (its evaluator's trace, its field multiplication), for the small sizes over Fq also against the
    witness the specification circuit allocates on the oracle's CS; the fill around the output survives."""
    m = o.modulus(field)
    st = mont([o.rand_fe(50 + t, 0, m), o.rand_fe(50 + t, 1, m), 9], m)
    tr, i_end, want = forward_segment_expected(cref, field, st, t)
    pad = 7
    buf = dev(np.full((3 * t + 1 + 2 * pad, 4), FILL, dtype="<u8"))
    ctx.minroot_forward_segment(field, dev(tr), t, i_end.copy(), buf[pad:])
    ctx.sync()
    got = host(buf)
    assert np.array_equal(got[pad:pad + 3 * t + 1], want)
    assert np.all(got[:pad] == FILL) and np.all(got[pad + 3 * t + 1:] == FILL)
    if field == o.FIELD_FQ and t <= 5:
        s0 = o.State(*unmont(st, m))
        cs = nv.CS(field)
        z = [cs.alloc_io(v) for v in (s0.x, s0.y, s0.i)]
        ForwardMinRootCircuit(t, s0, o.minroot_eval(s0, t, field)).synthesize(cs, z)
        assert unmont(got[pad:pad + 3 * t + 1], m) == cs.W
    with pytest.raises(VdfError):
        ctx.minroot_forward_segment(field, dev(tr), t, dev(i_end), buf[pad:])            # i_end is a host operand
    with pytest.raises(VdfError):
        ctx.minroot_forward_segment(field, tr, t, i_end.copy(), buf[pad:])               # the trace is a device operand


def spec_shape(t, before=2, after=3):
    """The specification circuit alone on the oracle's CS, z_in as three variables in front of the rounds, with a few other
    constraints before and after its rows: (shape, first round variable, first stencil row)."""
    cs = nv.CS(o.FIELD_FQ)
    z = [cs.alloc(0) for _ in range(3)]
    for _ in range(before):
        cs.enforce(z[0], z[1], z[2])
    ForwardMinRootCircuit(t, None, None).synthesize(cs, z)
    for _ in range(after):
        cs.enforce(z[2], z[1], cs.add(z[0], cs.const(3)))
    return cs.shape(), 3, before


@pytest.mark.parametrize("t", [1, 5, 1024, 65536])
def test_forward_stencil_equals_the_sparse_kernel(ctx, t):
    """vdf_nifs_cross_term_minroot_forward against vdf_nifs_cross_term_rows(.., VDF_ROWS_INSIDE) over the shape the
    specification circuit records: the same random z2 (constant column random, then ONE), random running vectors; A z2, B z2,
    C z2 and T equal, every row outside the range untouched."""
    from test_gpu_field_vec import _shape_arrays
    field, m = o.FIELD_FQ, o.Q
    sh, S, row0 = spec_shape(t)
    nr = 3 * t + 1
    nc, ncols = sh.num_cons, sh.num_vars + 1
    assert sh.num_vars == 3 + nr and nc == nr + 5
    shape = ctx.shape_create(field, nc, ncols, [_shape_arrays(e, m) for e in (sh.A, sh.B, sh.C)])
    rng = np.random.default_rng(7 * t + 1)
    abc1 = [dev(rand_limbs(rng, nc)) for _ in range(3)]
    u1 = rand_limbs(rng, 1)
    for unit in (False, True):
        z2 = rand_limbs(rng, ncols)
        if unit:
            z2[sh.num_vars] = limbs([o.to_mont(1, m)])[0]
        else:
            assert unmont(z2[sh.num_vars:], m) != [1]
        want = [dev(np.full((nc, 4), FILL, dtype="<u8")) for _ in range(4)]
        got = [dev(np.full((nc, 4), FILL, dtype="<u8")) for _ in range(4)]
        ctx.nifs_cross_term_rows(shape, row0, nr, 1, dev(z2), *abc1, u1, *want)
        ctx.nifs_cross_term_minroot_forward(field, t, S, sh.num_vars, row0, dev(z2), *abc1, u1, *got)
        ctx.sync()
        for k, (g, w) in enumerate(zip(got, want)):
            g, w = host(g), host(w)
            assert np.array_equal(g[row0:row0 + nr], w[row0:row0 + nr]), (unit, "ABCT"[k])
            assert np.all(g[:row0] == FILL) and np.all(g[row0 + nr:] == FILL), (unit, "ABCT"[k])
    with pytest.raises(VdfError):
        ctx.nifs_cross_term_minroot_forward(field, t, S, sh.num_vars - 1, row0, dev(z2), *abc1, u1, *got)   # the constant inside the rounds
    with pytest.raises(VdfError):
        ctx.nifs_cross_term_minroot_forward(field, t, 2, sh.num_vars, row0, dev(z2), *abc1, u1, *got)       # no room for z_in
    with pytest.raises(VdfError):
        ctx.nifs_cross_term_minroot_forward(field, t, S, sh.num_vars, row0, dev(z2), *abc1, dev(u1), *got)  # u1 is a host operand
    shape.free()


# ---- proofs against the oracle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("t,n", [(5, 3), (24, 2)])
def test_prove_steps_replayed_by_the_oracle(ctx, t, n):
    """Every step's fresh and running instances with their witnesses, both cross-term commitments and both challenges equal
    oracle.nova.prove_step's over the specification circuit; verify(z0 = initial, zi = final) passes; a swapped z0 / zi, a
    wrong step count and a tampered witness are refused."""
    pp, z0, fc, states, traces, init_ints = forward_chain(ctx, t, n, seed=77, i0=1)
    com = nv.CCommit()
    opp = oracle_pp(t, com)
    assert pp.digest() == opp.params
    for side in (0, 1):
        sz, sh = pp.sizes(side), opp.shapes[side]
        assert (sz["num_cons"], sz["num_vars"], sz["num_io"], sz["nnz"]) == (sh.num_cons, sh.num_vars, 2, len(sh.A) + len(sh.B) + len(sh.C))
    ost = chain(o.State(*init_ints), t, n)
    assert [s.to_ints(FIELD_FQ) for s in states] == [(s.x, s.y, s.i) for s in ost]
    z0i = [ost[0].x, ost[0].y, ost[0].i]
    proof, want = None, None
    for k in range(n):
        proof = NovaVDFProof.prove_step(pp, proof, fc, k, z0)
        want = nv.prove_step(opp, want, ForwardMinRootCircuit(t, ost[k], ost[k + 1]), z0i)
        tr, ls = want.trace[-1], proof.last_step()
        assert aff_ints(ls["comm_W1"], 0) == tuple(tr["l1"].comm_W) and unmont(ls["X1"], o.Q) == tr["l1"].X
        if k:
            assert aff_ints(ls["comm_T1"], 0) == tuple(tr["T1"]) and aff_ints(ls["comm_T2"], 1) == tuple(tr["T2"])
            assert (ls["r1"], ls["r2"]) == (tr["r1"], tr["r2"])
        check_instance(proof, INST_RUNNING_PRIMARY, 0, want.r[0])
        check_instance(proof, INST_RUNNING_SECONDARY, 1, want.r[1])
        check_instance(proof, INST_FRESH_SECONDARY, 1, want.l2)
        zp, zs = proof.zi()
        assert unmont(zp, o.Q) == want.zi[0] == [ost[k + 1].x, ost[k + 1].y, ost[k + 1].i] and unmont(zs, o.P) == want.zi[1]
        assert nv.verify(opp, want, k + 1, z0i) is not None
    zi = zvec(states[n])
    assert z0 == zvec(states[0])
    assert proof.verify(pp, n, z0, zi) is True
    assert proof.verify(pp, n, zi, z0) is False                       # the inverse kinds' reading of the same chain
    assert proof.verify(pp, n + 1, z0, zi) is False and proof.verify(pp, n - 1, z0, zi) is False
    assert proof.verify(pp, n, z0, [zi[1], zi[0], zi[2]]) is False
    # one word of a witness on the device
    seg_b, seg_n = pp.segment()
    assert seg_n == 3 * t + 1
    for which in (INST_RUNNING_PRIMARY, INST_RUNNING_SECONDARY, INST_FRESH_SECONDARY):
        dz, dE = C.c_void_p(), C.c_void_p()
        assert nova_lib.vdf_nova_proof_witness_ptrs(proof.handle, which, C.byref(dz), C.byref(dE)) == 0
        spots = [(dz.value, 32 * 40), (dE.value, 32 * 11)]
        if which == INST_RUNNING_PRIMARY:
            spots.append((dz.value, 32 * (seg_b + 3)))                # x_2, the second round's fifth root, of the folded witness
        for base, off in spots:
            if not base:
                continue
            word = np.zeros(1, dtype="<u8")
            ctx._check(lib.vdf_dev_memcpy(ctx.handle, word.ctypes.data, base + off, 8))
            bad = word ^ np.uint64(1)
            ctx._check(lib.vdf_dev_memcpy(ctx.handle, base + off, bad.ctypes.data, 8))
            assert proof.verify(pp, n, z0, zi) is False
            ctx._check(lib.vdf_dev_memcpy(ctx.handle, base + off, word.ctypes.data, 8))
            assert proof.verify(pp, n, z0, zi) is True
    proof.free(); fc.free(); pp.free()


def test_parameters_and_circuits_of_different_directions_do_not_mix(ctx):
    t = 8
    pp, z0, fc, states, traces, _ = forward_chain(ctx, t, 2, seed=3)
    ppb = public_params(ctx, t, CIRCUIT_MINROOT_BOUND)
    z0b, inv = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new_with_mode(FAST), t, 2, states[0])
    with pytest.raises(VdfError):
        NovaVDFProof.prove_step(pp, None, inv, 0, z0b)
    with pytest.raises(VdfError):
        NovaVDFProof.prove_step(ppb, None, fc, 0, z0)
    with pytest.raises(VdfError):
        NovaVDFProof.prove_step(pp, None, fc, 1, z0)                  # step 1 first: z0 is not its input
    with pytest.raises(VdfError):
        NovaVDFProof.eval_and_prove(ppb, PallasVDF.new_with_mode(FAST), states[0], 2)
    # fold_fused has no forward kernel: the parameters are made and the proof is the unfused one
    ppf = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD, fold_fused=1)
    a = NovaVDFProof.prove_recursively(pp, fc, t, z0)
    b = NovaVDFProof.prove_recursively(ppf, fc, t, z0)
    assert a.serialize() == b.serialize() and b.verify(ppf, 2, z0, zvec(states[2]))
    for h in (a, b, fc, inv, pp, ppb, ppf):
        h.free()


def test_stencil_at_full_size_and_one_fold_replayed_by_the_c_oracle(ctx, cref):
    """t = 2^16 over 3 steps with generators of known discrete logarithm: the parameters report stencil code 5; the running
    proof's wire bytes under stencil = 1 equal those under stencil = 0 (the generic sparse kernel); and the LAST fold is
    replayed by the C restatement over the ORACLE's shape of the specification circuit, as the inverse kinds' config 3 is:
    the rounds of the fresh witness, commitments by the discrete-log identity, A z, B z, C z, T, W' and E' element for element."""
    t, n = 1 << 16, 3
    L, fld, m = cref.lib(), o.FIELD_FQ, o.Q
    pp, z0, fc, states, traces, init_ints = forward_chain(ctx, t, n, seed=3, i0=1, family=GENS_KNOWN_DLOG)
    tn = pp.tuning()
    if not (tn["stencil"] == 1 and tn["early_rows"] != 0):
        pytest.skip("the environment overrides the defaults under test (tools/gpu_env_matrix.sh)")
    assert pp.stencil() == STENCIL_FORWARD == 5 and pp.early_rows()[1] == 3 * t + 1
    opp = oracle_pp(t, None, nv.FAMILY_KNOWN_DLOG)
    assert pp.digest() == opp.params
    sh = opp.shapes[0]
    nvar, nc = sh.num_vars, sh.num_cons
    seg_b, seg_n = pp.segment()
    assert seg_n == 3 * t + 1 and seg_b + seg_n <= nvar
    proof = None
    for k in range(n - 1):
        proof = NovaVDFProof.prove_step(pp, proof, fc, k, z0)
    z_old, E_old = proof.witness(INST_RUNNING_PRIMARY)
    inst_old = proof.instance(INST_RUNNING_PRIMARY)
    proof = NovaVDFProof.prove_step(pp, proof, fc, n - 1, z0)
    ls = proof.last_step()
    z2, _ = proof.witness(INST_FRESH_PRIMARY_LAST)
    z_new, E_new = proof.witness(INST_RUNNING_PRIMARY)
    inst_new = proof.instance(INST_RUNNING_PRIMARY)
    # the rounds of the fresh witness from the host evaluator's trace by the C restatement's multiplication
    xs = np.ascontiguousarray(traces[n - 1].reshape(t + 1, 2, 4)[1:, 0, :])
    sq, qd = cref.fe_array(t), cref.fe_array(t)
    L.ref_fe_mul(fld, cref.p(xs), cref.p(xs), t, cref.p(sq))
    L.ref_fe_mul(fld, cref.p(sq), cref.p(sq), t, cref.p(qd))
    i_end = np.frombuffer(states[n].i, dtype="<u8").reshape(1, 4)
    assert np.array_equal(z2[seg_b:seg_b + seg_n], np.concatenate([np.stack([xs, sq, qd], axis=1).reshape(3 * t, 4), i_end]))
    assert np.array_equal(z2[seg_b - 3:seg_b], np.frombuffer(b"".join(zvec(states[n - 1])), dtype="<u8").reshape(3, 4))     # z_in
    assert unmont(z2[nvar:nvar + 1], m) == [1] and np.array_equal(z2[nvar + 1:], ls["X1"])
    dl = lambda vec: o.msm_by_dlog_limbs(_canon(cref, fld, np.ascontiguousarray(vec)), o.CURVE_PALLAS, nv.GENS_SEED) or (0, 0)
    assert aff_ints(ls["comm_W1"], 0) == dl(z2[:nvar])

    def coo(mat):
        rows = np.array([e[0] for e in mat], dtype=np.uint32)
        cols = np.array([e[1] for e in mat], dtype=np.uint32)
        return rows, cols, limbs([o.to_mont(e[2], m) for e in mat])
    mats = [coo(x) for x in (sh.A, sh.B, sh.C)]

    def mv(z):
        out = []
        for rows, cols, vals in mats:
            e = cref.fe_array(nc)
            L.ref_spmv(fld, cref.p(rows), cref.p(cols), cref.p(vals), len(rows), cref.p(np.ascontiguousarray(z)), nc, cref.p(e))
            out.append(e)
        return out
    abc1, abc2 = mv(z_old), mv(z2)
    T = cref.fe_array(nc)
    L.ref_cross_term(fld, *(cref.p(x) for x in abc1 + abc2), cref.p(np.ascontiguousarray(inst_old["u"].reshape(1, 4))), nc, cref.p(T))
    assert aff_ints(ls["comm_T1"], 0) == dl(T)
    r = limbs([o.to_mont(ls["r1"], m)])
    W_exp, E_exp = cref.fe_array(nvar + 3), cref.fe_array(nc)
    L.ref_axpy(fld, cref.p(np.ascontiguousarray(z_old)), cref.p(r), cref.p(np.ascontiguousarray(z2)), nvar + 3, cref.p(W_exp))
    L.ref_axpy(fld, cref.p(np.ascontiguousarray(E_old)), cref.p(r), cref.p(T), nc, cref.p(E_exp))
    assert np.array_equal(z_new, W_exp) and np.array_equal(E_new, E_exp)
    assert np.array_equal(z_new[nvar], inst_new["u"]) and np.array_equal(z_new[nvar + 1:], inst_new["X"])
    assert aff_ints(inst_new["comm_W"], 0) == dl(z_new[:nvar]) and aff_ints(inst_new["comm_E"], 0) == dl(E_new)
    zi = zvec(states[n])
    assert proof.verify(pp, n, z0, zi)
    wire = proof.serialize()
    proof.free()
    # the same chain through the generic sparse kernel
    pp0 = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD, GENS_KNOWN_DLOG, stencil=0)
    assert pp0.stencil() == 0 and pp0.early_rows() == pp.early_rows() and pp0.digest() == pp.digest()
    b = NovaVDFProof.prove_recursively(pp0, fc, t, z0)
    assert b.serialize() == wire
    b.free(); pp0.free(); fc.free(); pp.free()


# ---- one chain, five ways ---------------------------------------------------------------------------------------

def test_one_chain_proved_five_ways_gives_one_proof(ctx):
    """(a) every step pushed as a trace, then prove_recursively; (b) push one, prove one, release one; (c) push_checkpoints with
    every = t and with every = t / 4, then materialize; (d) prove_recursively with a window of 2 over checkpoint steps never
    materialised; (e) eval_and_prove -- one set of wire bytes.  A checkpoint changed in one limb is reported by the step that
    ends at it."""
    t, n = 64, 5
    pp, z0, fc, states, traces, _ = forward_chain(ctx, t, n, seed=19, i0=2)
    zi = zvec(states[n])
    vdf = PallasVDF.new_with_mode(FAST)
    a = NovaVDFProof.prove_recursively(pp, fc, t, z0)
    assert a.verify(pp, n, z0, zi)
    wire = a.serialize()
    # (b)
    z0b, fb = ForwardCircuits.begin(t, states[0])
    b = None
    for k in range(n):
        fb.push_trace(traces[k])
        b = NovaVDFProof.prove_step(pp, b, fb, k, z0b)
        fb.release(k, 1)
        assert fb.host_bytes() == 0
    assert z0b == z0 and b.serialize() == wire
    # (c), (d)
    for every in (t, t // 4):
        cps = vdf.eval_checkpoints(states[0], t * n, every)
        per = t // every
        z0c, fcp = ForwardCircuits.begin(t, states[0])
        for k in range(n):
            fcp.push_checkpoints(every, cps[k * per:(k + 1) * per + 1])
        assert len(fcp) == n and fcp.states(n - 1) == (states[n], states[n - 1]) and fcp.memory() == (0, 0)
        with pytest.raises(VdfError):
            NovaVDFProof.prove_step(pp, None, fcp, 0, z0c)             # no trace yet
        assert fcp.materialize(ctx) == [0] * n and fcp.memory()[0] == n
        # a rebuilt trace is the evaluator's
        got = np.zeros((t + 1) * 8, dtype="<u8")
        assert lib.vdf_dev_memcpy(ctx.handle, got.ctypes.data, fcp.trace_ptr(2), got.nbytes) == 0
        assert np.array_equal(got.reshape(-1, 4), traces[2])
        c = NovaVDFProof.prove_recursively(pp, fcp, t, z0c)
        assert c.serialize() == wire
        fcp.release()
        assert fcp.memory() == (0, 0)
        d = NovaVDFProof.prove_recursively(pp, fcp, t, z0c, window_steps=2)
        assert d.serialize() == wire and fcp.memory() == (0, 0)
        c.free(); d.free(); fcp.free()
    # (e)
    e, final, stats = NovaVDFProof.eval_and_prove(pp, vdf, states[0], n)
    assert final == states[n] and e.serialize() == wire and e.verify(pp, n, z0, zi)
    assert stats["steps"] == n and 1 <= stats["max_backlog"] <= n and stats["eval_ms"] > 0 and stats["after_eval_ms"] > 0
    # a checkpoint changed in one limb
    every, per = t // 4, 4
    cps = vdf.eval_checkpoints(states[0], t * n, every)
    for step, idx in ((1, 2), (n - 1, per)):                           # inside step 1; the state the last step ends at
        z0t, ft = ForwardCircuits.begin(t, states[0])
        for k in range(n):
            part = list(cps[k * per:(k + 1) * per + 1])
            if k == step:
                x = bytearray(part[idx].x)
                x[9] ^= 0x10
                part[idx] = State(bytes(x), part[idx].y, part[idx].i)
            ft.push_checkpoints(every, part)
        with pytest.raises(VdfError) as err:
            ft.materialize(ctx)
        assert ft.last_bad == [1 if k == step else 0 for k in range(n)] and ("circuit %d" % step) in str(err.value)
        ft.free()
    for h in (a, b, e, fb, fc, pp):
        h.free()


# ---- the wire and the batch calls -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_forward():
    with open(os.path.join(ROOT, "tests", "golden", "forward.json")) as f:
        return json.load(f)


def test_wire_and_batches(ctx, golden_forward):
    """compress -> wire -> deserialize under a second context -> verify_compressed; the SHA-256 of the "VDFSNK03" bytes for
    (t, steps) = (5, 3) is the oracle-derived one of tests/golden/forward.json (so is the running proof's); the two batch
    verifiers and compress_batch take forward proofs under forward parameters."""
    g = golden_forward["wire_t5_n3"]
    t, n = g["t"], g["steps"]
    pp, z0, fc, states, traces, _ = forward_chain(ctx, t, n, seed=g["seed"], i0=g["i0"])
    assert pp.digest() == int(g["params"], 16)
    zi = zvec(states[n])
    proof = NovaVDFProof.prove_recursively(pp, fc, t, z0)
    running = proof.serialize()
    assert len(running) == g["running_proof_len"] and hashlib.sha256(running).hexdigest() == g["running_proof_sha256"]
    snark = proof.compress(pp)
    wire = snark.serialize()
    assert wire[:8] == b"VDFSNK03" and len(wire) == g["compressed_proof_len"]
    assert hashlib.sha256(wire).hexdigest() == g["compressed_proof_sha256"]
    assert snark.verify(pp, n, z0, zi) and not snark.verify(pp, n, zi, z0) and not snark.verify(pp, n + 1, z0, zi)
    ctx2 = vdf_amd.Context(0)
    pp2 = public_params(ctx2, t, CIRCUIT_MINROOT_FORWARD)
    again = CompressedNovaVDFProof.deserialize(pp2, wire)
    assert again.verify(pp2, n, z0, zi) and again.serialize() == wire
    resumed = NovaVDFProof.deserialize(pp2, running)
    assert resumed.verify(pp2, n, z0, zi) and resumed.serialize() == running
    ppb = public_params(ctx2, t, CIRCUIT_MINROOT_BOUND)               # other parameters refuse the bytes
    with pytest.raises(VdfError):
        CompressedNovaVDFProof.deserialize(ppb, wire)
    for h in (again, resumed, pp2, ppb):
        h.free()
    ctx2.close()
    # a second, longer chain under the same parameters for the batches
    vdf = PallasVDF.new_with_mode(FAST)
    p2, fin2, _ = NovaVDFProof.eval_and_prove(pp, vdf, states[1], 4)
    z0_2, zi_2 = zvec(states[1]), zvec(fin2)
    assert verify_batch(pp, [(proof, n, z0, zi), (p2, 4, z0_2, zi_2), (proof, n, zi, z0), (p2, 3, z0_2, zi_2)]) == [True, True, False, False]
    snarks = compress_batch(pp, [proof, p2])
    assert snarks[0].serialize() == wire and snarks[1].serialize() == p2.compress(pp).serialize()
    assert verify_compressed_batch(pp, [(snarks[0], n, z0, zi), (snarks[1], 4, z0_2, zi_2), (snarks[1], 4, z0, zi_2)]) == [True, True, False]
    for h in snarks + [snark, proof, p2, fc, pp]:
        h.free()


# ---- the plain-C client ----------------------------------------------------------------------------------------

def test_prove_stream_client(tmp_path):
    """examples/prove_stream (plain C over the two ABIs) as a fresh child process at t = 1,024 over 8 steps: exit 0, every
    verification as expected, and the final state it proved is vdf_minroot_eval's."""
    exe = os.path.join(ROOT, "examples", "prove_stream")
    assert os.path.exists(exe), "examples/prove_stream is built by vdf_amd/csrc/Makefile (all)"
    out_path = str(tmp_path / "wire.bin")
    # a fresh child process (never an exec of this one)
    r = subprocess.run([exe, "10", "8", "123", "0", out_path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true" and lines["verify with z0 and zi swapped"] == "false"
    assert "decoded and verified: true" in r.stdout and "stencil code 5" in r.stdout
    want = PallasVDF.new_with_mode(FAST).eval(State.from_ints(FIELD_FQ, 123, 0, 0), 1024 * 8)
    assert bytes.fromhex(lines["final state"]) == want.x + want.y + want.i
    assert open(out_path, "rb").read()[:8] == b"VDFSNK03"
