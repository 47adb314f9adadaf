"""GPU: the curve cycle in the other orientation (include/vdf_nova.h vdf_nova_public_params_field(VDF_FIELD_FP)): the primary
circuit over Fp, G1 = Vesta, G2 = Pallas -- proofs of VestaVDF chains.  Whole proofs against oracle/nova.py with its two
orientation tuples exchanged (tests/vesta_spec.py): every step's instances and witnesses, lanes, checkpoints and windows,
eval_and_prove, compress and both wire formats, the batch calls, the refusals between orientations, two orientations
interleaved in one process, one fold at full size by the C restatement, a custom circuit over Fp, and the plain-C client.
Every comparison is of bytes."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import vdf_amd
from oracle import nova as nv, pasta as o, wire
import vesta_spec as vs
from test_gpu_nova import _canon
from util import limbs, unmont
from vdf_amd._lib import lib
from vdf_amd.hip import VdfError
from vdf_amd.minroot import EvalMode, PallasVDF, VestaVDF, State, FIELD_FP, FIELD_FQ
from vdf_amd.nova import (CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_REFERENCE, CIRCUIT_MINROOT_FORWARD, STENCIL_FORWARD, GENS_KNOWN_DLOG,
                          GENS_TRY_AND_INCREMENT, INST_RUNNING_PRIMARY, INST_RUNNING_SECONDARY, INST_FRESH_SECONDARY, INST_FRESH_PRIMARY_LAST,
                          CompressedNovaVDFProof, ForwardCircuits, InverseMinRootCircuit, LaneCircuits, NovaVDFProof, StepCircuit,
                          compress_batch, nova_lib, public_params, public_params_custom, public_params_lanes, verify_batch,
                          verify_compressed_batch)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = EvalMode.LTRAddChainSequential
FP, FQ = o.FIELD_FP, o.FIELD_FQ
BASE = (o.Q, o.P)                      # coordinate modulus of side 0 / 1 commitments in the Fp orientation (Vesta / Pallas)
SCAL = (o.P, o.Q)                      # scalar modulus of side 0 / 1 instances
ERR_BAD_ARG, ERR_NONCANONICAL = 1, 3


def zvec(s):
    return [s.x, s.y, s.i]


def aff_ints(arr, side):
    return tuple(unmont(np.asarray(arr).reshape(2, 4), BASE[side]))


def check_instance(proof, which, side, want):
    """instance + witness of the product against an oracle Relaxed / Fresh (tests/test_gpu_nova.py's, for this orientation)"""
    m = SCAL[side]
    inst = proof.instance(which)
    z, E = proof.witness(which)
    assert aff_ints(inst["comm_W"], side) == tuple(want.comm_W)
    assert unmont(inst["X"], m) == list(want.X)
    zz = unmont(z, m)
    nvars = len(want.W)
    assert zz[:nvars] == list(want.W)
    if which == INST_FRESH_SECONDARY:
        assert zz[nvars:] == [1] + list(want.X) and E is None
        assert unmont(inst["u"].reshape(1, 4), m) == [1] and aff_ints(inst["comm_E"], side) == (0, 0)
    else:
        assert aff_ints(inst["comm_E"], side) == tuple(want.comm_E)
        assert unmont(inst["u"].reshape(1, 4), m) == [want.u]
        assert zz[nvars:] == [want.u] + list(want.X)
        assert unmont(E, m) == list(want.E)


def check_step(proof, want, k):
    tr, ls = want.trace[-1], proof.last_step()
    assert aff_ints(ls["comm_W1"], 0) == tuple(tr["l1"].comm_W) and unmont(ls["X1"], o.P) == tr["l1"].X
    if k:
        assert aff_ints(ls["comm_T1"], 0) == tuple(tr["T1"]) and aff_ints(ls["comm_T2"], 1) == tuple(tr["T2"])
        assert (ls["r1"], ls["r2"]) == (tr["r1"], tr["r2"])
    check_instance(proof, INST_RUNNING_PRIMARY, 0, want.r[0])
    check_instance(proof, INST_RUNNING_SECONDARY, 1, want.r[1])
    check_instance(proof, INST_FRESH_SECONDARY, 1, want.l2)


def vesta_chain(ctx, kind, t, n, seed=42, i0=0, family=GENS_TRY_AND_INCREMENT, **tune):
    """(pp over Fp, z0, circuits, [State] at the step boundaries, the traces, the initial state as ints) of a VestaVDF chain:
    a forward chain with every trace pushed for the forward kind, eval_and_make_circuits (reversed) for the inverse kinds"""
    x = o.rand_fe(seed, 0, o.P)
    initial = State.from_ints(FIELD_FP, x, 0, i0)
    pp = public_params(ctx, t, kind, family, field=FIELD_FP, **tune)
    assert pp.field() == FIELD_FP
    vdf = VestaVDF.new_with_mode(FAST)
    states, traces = [initial], []
    for _ in range(n):
        s, tr = vdf.eval_with_trace(states[-1], t)
        states.append(s)
        traces.append(tr)
    if kind == CIRCUIT_MINROOT_FORWARD:
        z0, c = ForwardCircuits.begin(t, initial, field=FIELD_FP)
        for tr in traces:
            c.push_trace(tr)
    else:
        z0, c = InverseMinRootCircuit.eval_and_make_circuits(vdf, t, n, initial)
    assert c.field() == FIELD_FP
    return pp, z0, c, states, traces, (x, 0, i0)


def pallas_chain(ctx, t, n, seed=42, i0=0):
    x = o.rand_fe(seed, 0, o.Q)
    initial = State.from_ints(FIELD_FQ, x, 0, i0)
    pp = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD)
    vdf = PallasVDF.new_with_mode(FAST)
    z0, c = ForwardCircuits.begin(t, initial)
    states = [initial]
    for _ in range(n):
        s, tr = vdf.eval_with_trace(states[-1], t)
        states.append(s)
        c.push_trace(tr)
    assert pp.field() == FIELD_FQ and c.field() == FIELD_FQ
    return pp, z0, c, states


# ---- 1. steps replayed by the oracle --------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,t,n", [(CIRCUIT_MINROOT_FORWARD, 5, 3), (CIRCUIT_MINROOT_FORWARD, 24, 2), (CIRCUIT_MINROOT_REFERENCE, 5, 3),
                                      (CIRCUIT_MINROOT_BOUND, 5, 3)], ids=["forward-5x3", "forward-24x2", "reference-5x3", "bound-5x3"])
def test_prove_steps_replayed_by_the_swapped_oracle(ctx, kind, t, n):
    """Every step's fresh and running instances with their witnesses, both cross-term commitments and both challenges equal the
    swapped oracle's; verify passes, and fails for a wrong z0 and for a wrong zi."""
    pp, z0, circ, states, traces, init_ints = vesta_chain(ctx, kind, t, n, seed=77, i0=1)
    forward = kind == CIRCUIT_MINROOT_FORWARD
    with vs.swapped():
        opp = vs.oracle_pp(FP, kind, t, commit=nv.CCommit())
        assert pp.digest() == opp.params
        for side in (0, 1):
            sz, sh = pp.sizes(side), opp.shapes[side]
            assert (sz["num_cons"], sz["num_vars"], sz["num_io"], sz["nnz"]) == (sh.num_cons, sh.num_vars, 2, len(sh.A) + len(sh.B) + len(sh.C))
        ost = vs.chain(FP, o.State(*init_ints), t, n)
        assert [s.to_ints(FIELD_FP) for s in states] == [(s.x, s.y, s.i) for s in ost]
        first = ost[0] if forward else ost[n]
        z0i = [first.x, first.y, first.i]
        proof, want = None, None
        for k in range(n):
            proof = NovaVDFProof.prove_step(pp, proof, circ, k, z0)
            if forward:
                step, now = vs.ForwardMinRootCircuit(FP, t, ost[k], ost[k + 1]), ost[k + 1]
            else:
                step, now = nv.InverseMinRootCircuit(t, ost[n - k], ost[n - k - 1], kind == CIRCUIT_MINROOT_BOUND), ost[n - k - 1]
            want = nv.prove_step(opp, want, step, z0i)
            check_step(proof, want, k)
            zp, zs = proof.zi()
            assert unmont(zp, o.P) == want.zi[0] == [now.x, now.y, now.i] and unmont(zs, o.Q) == want.zi[1]
        assert nv.verify(opp, want, n, z0i) is not None
    assert nv.SIDE_FIELD == (FQ, FP)
    last = states[n] if forward else states[0]
    zi = zvec(last)
    assert z0 == zvec(states[0] if forward else states[n])
    assert proof.verify(pp, n, z0, zi) is True
    assert proof.verify(pp, n, [zi[0], z0[1], z0[2]], zi) is False     # a wrong z0
    assert proof.verify(pp, n, z0, [zi[1], zi[0], zi[2]]) is False     # a wrong zi
    assert proof.verify(pp, n + 1, z0, zi) is False
    proof.free(); circ.free(); pp.free()


# ---- 2. lanes -------------------------------------------------------------------------------------------------------

def test_lanes_replayed_by_the_swapped_oracle(ctx):
    t, n, L = 5, 2, 3
    ints = [(o.rand_fe(11 + l, 0, o.P), l, 7 * l) for l in range(L)]
    initials = [State.from_ints(FIELD_FP, *v) for v in ints]
    pp = public_params_lanes(ctx, t, L, field=FIELD_FP)
    assert pp.field() == FIELD_FP and pp.lanes() == L
    vdf = VestaVDF.new_with_mode(FAST)
    z0, lc = LaneCircuits.begin(t, initials, field=FIELD_FP)
    cur = list(initials)
    for _ in range(n):
        res = [vdf.eval_with_trace(s, t) for s in cur]
        lc.push_traces([r[1] for r in res])
        cur = [r[0] for r in res]
    with vs.swapped():
        opp = vs.oracle_pp(FP, vs.LANES, t, L, commit=nv.CCommit())
        assert pp.digest() == opp.params
        sts = vs.chains(FP, [o.State(*v) for v in ints], t, n)
        z0i = vs.flat(sts[0])
        proof, want = None, None
        for k in range(n):
            proof = NovaVDFProof.prove_step(pp, proof, lc, k, z0)
            want = nv.prove_step(opp, want, vs.LanesForwardCircuit(FP, t, sts[k], sts[k + 1]), z0i)
            check_step(proof, want, k)
            assert unmont(proof.zi()[0], o.P) == want.zi[0] == vs.flat(sts[k + 1])
    zi = [v for s in cur for v in zvec(s)]
    assert proof.verify(pp, n, z0, zi) is True and proof.verify(pp, n, z0, zi[3:] + zi[:3]) is False
    proof.free(); lc.free(); pp.free()


# ---- 3. checkpoints and windows ---------------------------------------------------------------------------------------

def test_checkpoints_and_windows_over_fp(ctx):
    """t = 64, every = 16, 5 steps: the inverse walks and the landing check on the device run over Fp.  The windowed prover over
    from_checkpoints(field = FP) gives the bytes of the same chain proved from host traces; a corrupted checkpoint is reported."""
    t, every, n = 64, 16, 5
    pp, z0, circ, states, traces, _ = vesta_chain(ctx, CIRCUIT_MINROOT_REFERENCE, t, n, seed=19, i0=2)
    a = NovaVDFProof.prove_recursively(pp, circ, t, z0)
    assert a.verify(pp, n, z0, zvec(states[0]))
    want = a.serialize()
    vdf = VestaVDF.new_with_mode(FAST)
    cps = vdf.eval_checkpoints(states[0], t * n, every)
    z0c, cc = InverseMinRootCircuit.from_checkpoints(t, every, n, cps, field=FIELD_FP)
    assert z0c == z0 and cc.field() == FIELD_FP and cc.memory() == (0, 0)
    b = NovaVDFProof.prove_recursively(pp, cc, t, z0c, window_steps=2)
    assert b.serialize() == want and cc.memory() == (0, 0)
    # a rebuilt trace is the evaluator's: circuit n - 1 is the chain's first step
    assert cc.materialize(ctx, n - 1, 1) == [0]
    got = np.zeros((t + 1) * 8, dtype="<u8")
    assert lib.vdf_dev_memcpy(ctx.handle, got.ctypes.data, cc.trace_ptr(n - 1), got.nbytes) == 0
    assert np.array_equal(got.reshape(-1, 4), traces[0])
    # one limb of a checkpoint changed: the walks that meet it miss
    per = t // every
    bad = list(cps)
    x = bytearray(bad[per + 2].x)
    x[9] ^= 0x10
    bad[per + 2] = State(bytes(x), bad[per + 2].y, bad[per + 2].i)       # inside the chain's second step = circuit n - 2
    _, cb = InverseMinRootCircuit.from_checkpoints(t, every, n, bad, field=FIELD_FP)
    with pytest.raises(VdfError) as err:
        cb.materialize(ctx)
    assert cb.last_bad == [1 if k == n - 2 else 0 for k in range(n)] and ("circuit %d" % (n - 2)) in str(err.value)
    for h in (a, b, cc, cb, circ, pp):
        h.free()


# ---- 4. eval_and_prove -------------------------------------------------------------------------------------------------

def test_eval_and_prove_runs_the_parameters_field(ctx):
    t, n = 256, 4
    pp, z0, fc, states, traces, _ = vesta_chain(ctx, CIRCUIT_MINROOT_FORWARD, t, n, seed=5, i0=3)
    vdf = VestaVDF.new_with_mode(FAST)
    e, final, stats = NovaVDFProof.eval_and_prove(pp, vdf, states[0], n)
    assert final == states[n] == VestaVDF.new().eval(states[0], t * n) and stats["steps"] == n
    a = NovaVDFProof.prove_recursively(pp, fc, t, z0)
    assert e.serialize() == a.serialize() and e.verify(pp, n, z0, zvec(final))
    with pytest.raises(VdfError):                                        # a PallasVDF under these parameters
        NovaVDFProof.eval_and_prove(pp, PallasVDF.new_with_mode(FAST), states[0], n)
    for h in (a, e, fc, pp):
        h.free()


# ---- 5. compress, wire and batches -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_vesta():
    with open(os.path.join(ROOT, "tests", "golden", "vesta.json")) as f:
        return json.load(f)


def test_compress_wire_and_batches(ctx, golden_vesta):
    t, n = 5, 3
    pp, z0, fc, states, traces, init_ints = vesta_chain(ctx, CIRCUIT_MINROOT_FORWARD, t, n, seed=31, i0=0)
    zi = zvec(states[n])
    proof = NovaVDFProof.prove_recursively(pp, fc, t, z0)
    snark = proof.compress(pp)
    wire_bytes = snark.serialize()
    with vs.swapped():
        opp = vs.oracle_pp(FP, vs.FORWARD, t, commit=nv.CCommit())
        ost = vs.chain(FP, o.State(*init_ints), t, n)
        z0i = [ost[0].x, ost[0].y, ost[0].i]
        want = None
        for k in range(n):
            want = nv.prove_step(opp, want, vs.ForwardMinRootCircuit(FP, t, ost[k], ost[k + 1]), z0i)
        assert proof.serialize() == wire.encode_running_proof(t, opp.params, want, z0i)
        assert wire_bytes == wire.encode_compressed_proof(t, opp.params, nv.compress(opp, want))
    assert wire_bytes[:8] == b"VDFSNK03"
    assert snark.verify(pp, n, z0, zi) and not snark.verify(pp, n, zi, z0) and not snark.verify(pp, n + 1, z0, zi)
    # the committed hash: t = 2, 3 steps
    g = golden_vesta["wire_t2_n3"]
    ppg, z0g, fcg, stg, _, _ = vesta_chain(ctx, CIRCUIT_MINROOT_FORWARD, g["t"], g["steps"], seed=g["seed"], i0=g["i0"])
    assert ppg.digest() == int(g["params"], 16)
    pg = NovaVDFProof.prove_recursively(ppg, fcg, g["t"], z0g)
    wg = pg.compress(ppg).serialize()
    assert len(wg) == g["compressed_proof_len"] and hashlib.sha256(wg).hexdigest() == g["compressed_proof_sha256"]
    for h in (pg, fcg, ppg):
        h.free()
    # a second chain under the same parameters for the batches
    vdf = VestaVDF.new_with_mode(FAST)
    p2, fin2, _ = NovaVDFProof.eval_and_prove(pp, vdf, states[1], 4)
    z0_2, zi_2 = zvec(states[1]), zvec(fin2)
    snarks = compress_batch(pp, [proof, p2])
    assert snarks[0].serialize() == wire_bytes and snarks[1].serialize() == p2.compress(pp).serialize()
    assert verify_compressed_batch(pp, [(snarks[0], n, z0, zi), (snarks[1], 4, z0_2, zi_2)]) == [True, True]
    assert verify_batch(pp, [(proof, n, z0, zi), (p2, 4, z0_2, zi_2)]) == [True, True]
    flat = bytearray(snarks[1].to_bytes())
    flat[40] ^= 1                                                         # one bit of the primary argument of entry 1
    snarks[1].set_bytes(bytes(flat))
    assert verify_compressed_batch(pp, [(snarks[0], n, z0, zi), (snarks[1], 4, z0_2, zi_2)]) == [True, False]
    dz, dE = C.c_void_p(), C.c_void_p()
    assert nova_lib.vdf_nova_proof_witness_ptrs(p2.handle, INST_RUNNING_PRIMARY, C.byref(dz), C.byref(dE)) == 0
    word = np.zeros(1, dtype="<u8")
    ctx._check(lib.vdf_dev_memcpy(ctx.handle, word.ctypes.data, dz.value + 32 * 40, 8))
    ctx._check(lib.vdf_dev_memcpy(ctx.handle, dz.value + 32 * 40, (word ^ np.uint64(1)).ctypes.data, 8))
    assert verify_batch(pp, [(proof, n, z0, zi), (p2, 4, z0_2, zi_2)]) == [True, False]
    ctx._check(lib.vdf_dev_memcpy(ctx.handle, dz.value + 32 * 40, word.ctypes.data, 8))
    assert verify_batch(pp, [(proof, n, z0, zi), (p2, 4, z0_2, zi_2)]) == [True, True]
    # serialize -> deserialize under a second context -> prove_step goes on to the same bytes
    z0s, fs = ForwardCircuits.begin(t, states[0], field=FIELD_FP)
    for tr in traces:
        fs.push_trace(tr)
    part = None
    for k in range(n - 1):
        part = NovaVDFProof.prove_step(pp, part, fs, k, z0s)
    blob = part.serialize()
    ctx2 = vdf_amd.Context(0)
    pp2 = public_params(ctx2, t, CIRCUIT_MINROOT_FORWARD, field=FIELD_FP)
    resumed = NovaVDFProof.deserialize(pp2, blob)
    assert resumed.serialize() == blob
    resumed = NovaVDFProof.prove_step(pp2, resumed, fs, n - 1, z0s)
    assert resumed.serialize() == proof.serialize() and resumed.verify(pp2, n, z0, zi)
    again = CompressedNovaVDFProof.deserialize(pp2, wire_bytes)
    assert again.verify(pp2, n, z0, zi) and again.serialize() == wire_bytes
    for h in (again, resumed, pp2):
        h.free()
    ctx2.close()
    for h in snarks + [snark, part, proof, p2, fs, fc, pp]:
        h.free()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def test_orientations_do_not_mix(ctx):
    t, n = 5, 2
    ppv, z0v, fcv, stv, _, _ = vesta_chain(ctx, CIRCUIT_MINROOT_FORWARD, t, n, seed=9, i0=0)
    ppq, z0q, fcq, stq = pallas_chain(ctx, t, n, seed=9, i0=0)
    assert ppv.digest() != ppq.digest()
    pv = NovaVDFProof.prove_step(ppv, None, fcv, 0, z0v)
    pq = NovaVDFProof.prove_step(ppq, None, fcq, 0, z0q)
    before_v, before_q = pv.serialize(), pq.serialize()
    for pp, proof, circ, z0 in ((ppv, pv, fcq, z0q), (ppv, None, fcq, z0q), (ppq, pq, fcv, z0v), (ppq, None, fcv, z0v)):
        with pytest.raises(VdfError) as e:
            NovaVDFProof.prove_step(pp, proof, circ, 1 if proof is not None else 0, z0)
        assert e.value.code == ERR_BAD_ARG and "orientation" in str(e.value)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively(ppv, fcq, t, z0q)
    assert e.value.code == ERR_BAD_ARG
    assert pv.serialize() == before_v and pq.serialize() == before_q
    pv = NovaVDFProof.prove_step(ppv, pv, fcv, 1, z0v)
    pq = NovaVDFProof.prove_step(ppq, pq, fcq, 1, z0q)
    assert pv.verify(ppv, n, z0v, zvec(stv[n])) and pq.verify(ppq, n, z0q, zvec(stq[n]))
    blob_v, blob_q = pv.serialize(), pq.serialize()
    wire_v = pv.compress(ppv).serialize()
    # a blob of one orientation under parameters of the other
    for pp, blob in ((ppq, blob_v), (ppv, blob_q)):
        with pytest.raises(VdfError) as e:
            NovaVDFProof.deserialize(pp, blob)
        assert e.value.code == ERR_BAD_ARG
    with pytest.raises(VdfError) as e:
        CompressedNovaVDFProof.deserialize(ppq, wire_v)
    assert e.value.code == ERR_BAD_ARG
    # canonicity per side: the integer p is a canonical element of Fq and not of Fp (p < q).  "VDFRSK02": z_i primary at
    # 8 + 8 + 8 + 32 + 96 = 152
    assert o.P < o.Q and len(blob_v) == len(blob_q)
    word = o.P.to_bytes(32, "little")
    tv, tq = bytearray(blob_v), bytearray(blob_q)
    tv[152:184] = word
    tq[152:184] = word
    with pytest.raises(VdfError) as e:
        NovaVDFProof.deserialize(ppv, bytes(tv))
    assert e.value.code == ERR_NONCANONICAL
    accepted = NovaVDFProof.deserialize(ppq, bytes(tq))                   # canonical there: decoded (it states another z_i)
    assert accepted.serialize() == bytes(tq) and accepted.verify(ppq, n, z0q, zvec(stq[n])) is False
    for h in (accepted, pv, pq, fcv, fcq, ppv, ppq):
        h.free()


# ---- 7. two orientations in one process ------------------------------------------------------------------------------------------

def test_two_orientations_interleaved_on_one_context(ctx):
    t, n = 24, 3
    ppv, z0v, fcv, stv, _, _ = vesta_chain(ctx, CIRCUIT_MINROOT_FORWARD, t, n, seed=21, i0=4)
    ppq, z0q, fcq, stq = pallas_chain(ctx, t, n, seed=22, i0=5)
    solo_v = NovaVDFProof.prove_recursively(ppv, fcv, t, z0v)
    solo_q = NovaVDFProof.prove_recursively(ppq, fcq, t, z0q)
    want_v, want_q = solo_v.serialize(), solo_q.serialize()
    solo_v.free(); solo_q.free()
    pv = pq = None
    for k in range(n):
        pq = NovaVDFProof.prove_step(ppq, pq, fcq, k, z0q)
        pv = NovaVDFProof.prove_step(ppv, pv, fcv, k, z0v)
    assert pv.serialize() == want_v and pq.serialize() == want_q
    assert pv.verify(ppv, n, z0v, zvec(stv[n])) and pq.verify(ppq, n, z0q, zvec(stq[n]))
    assert pv.compress(ppv).verify(ppv, n, z0v, zvec(stv[n])) and pq.compress(ppq).verify(ppq, n, z0q, zvec(stq[n]))
    for h in (pv, pq, fcv, fcq, ppv, ppq):
        h.free()


# ---- 8. full size, once ------------------------------------------------------------------------------------------------------------

def test_full_size_over_fp_and_one_fold_replayed_by_the_c_oracle(ctx, cref):
    """t = 2^16 over 3 steps with generators of known discrete logarithm: the smallest t at which the Vesta side has 2^17
    generators and more, so that the big fixed-base window, the early rows' queue, the lookahead and the digit-table ranges run
    on that curve.  The parameters report stencil code 5 and early rows; the LAST fold is replayed by the C restatement over the
    swapped oracle's shape, commitments by the discrete-log identity on Vesta -- as tests/test_gpu_forward.py does over Fq."""
    t, n = 1 << 16, 3
    L, fld, m = cref.lib(), o.FIELD_FP, o.P
    pp, z0, fc, states, traces, init_ints = vesta_chain(ctx, CIRCUIT_MINROOT_FORWARD, t, n, seed=3, i0=1, family=GENS_KNOWN_DLOG)
    tn = pp.tuning()
    if not (tn["stencil"] == 1 and tn["early_rows"] != 0):
        pytest.skip("the environment overrides the defaults under test (tools/gpu_env_matrix.sh)")
    assert pp.stencil() == STENCIL_FORWARD == 5 and pp.early_rows()[1] == 3 * t + 1
    assert pp.sizes(0)["num_gens"] >= 1 << 17
    with vs.swapped():
        opp = vs.oracle_pp(FP, vs.FORWARD, t, family=nv.FAMILY_KNOWN_DLOG)
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
    xs = np.ascontiguousarray(traces[n - 1].reshape(t + 1, 2, 4)[1:, 0, :])
    sq, qd = cref.fe_array(t), cref.fe_array(t)
    L.ref_fe_mul(fld, cref.p(xs), cref.p(xs), t, cref.p(sq))
    L.ref_fe_mul(fld, cref.p(sq), cref.p(sq), t, cref.p(qd))
    i_end = np.frombuffer(states[n].i, dtype="<u8").reshape(1, 4)
    assert np.array_equal(z2[seg_b:seg_b + seg_n], np.concatenate([np.stack([xs, sq, qd], axis=1).reshape(3 * t, 4), i_end]))
    assert np.array_equal(z2[seg_b - 3:seg_b], np.frombuffer(b"".join(zvec(states[n - 1])), dtype="<u8").reshape(3, 4))     # z_in
    assert unmont(z2[nvar:nvar + 1], m) == [1] and np.array_equal(z2[nvar + 1:], ls["X1"])
    dl = lambda vec: o.msm_by_dlog_limbs(_canon(cref, fld, np.ascontiguousarray(vec)), o.CURVE_VESTA, nv.GENS_SEED) or (0, 0)
    assert aff_ints(ls["comm_W1"], 0) == dl(z2[:nvar])

    def coo(mat):
        rows = np.array([e[0] for e in mat], dtype=np.uint32)
        cols = np.array([e[1] for e in mat], dtype=np.uint32)
        return rows, cols, limbs([o.to_mont(e[2] % m, m) for e in mat])
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
    assert proof.verify(pp, n, z0, zvec(states[n]))
    wire_bytes = proof.serialize()
    proof.free()
    # the same chain through the generic sparse kernel
    pp0 = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD, GENS_KNOWN_DLOG, field=FIELD_FP, stencil=0)
    assert pp0.stencil() == 0 and pp0.early_rows() == pp.early_rows() and pp0.digest() == pp.digest()
    b = NovaVDFProof.prove_recursively(pp0, fc, t, z0)
    assert b.serialize() == wire_bytes
    b.free(); pp0.free(); fc.free(); pp.free()


# ---- 9. a custom circuit over Fp ------------------------------------------------------------------------------------------------------

def fe(v):
    return limbs([o.to_mont(v % o.P, o.P)]).tobytes()


class CubicFp(StepCircuit):
    arity = 1

    def synthesize(self, cs, z):
        x = z[0]
        x2 = cs.mul(x, x)
        x3 = cs.mul(x2, x)
        rhs = cs.add(cs.add(x3, x), cs.const(fe(5)))
        y = cs.alloc(cs.value(rhs) if cs.is_witness else None)
        cs.enforce(rhs, cs.const(fe(1)), y)
        return [y]


def test_a_custom_circuit_over_fp(ctx):
    n, x0 = 3, 0x1234567
    circuit = CubicFp()
    pp = public_params_custom(ctx, circuit, field=FIELD_FP)
    assert pp.field() == FIELD_FP and pp.segment() == (0, 0)
    z0 = [fe(x0)]
    with vs.swapped():
        opp = nv.public_params(0, nv.CCommit(), nv.GENS_SEED, nv.FAMILY_TRY_AND_INCREMENT, primary=vs.CubicCircuit(FP))
        assert pp.digest() == opp.params
        proof, want, x = None, None, x0
        for k in range(n):
            proof = NovaVDFProof.prove_step_custom(pp, proof, circuit, z0)
            want = nv.prove_step(opp, want, vs.CubicCircuit(FP), [x0])
            x = (x ** 3 + x + 5) % o.P
            check_step(proof, want, k)
            zp, zs = proof.zi()
            assert unmont(zp, o.P) == [x] == want.zi[0] and unmont(zs, o.Q) == [0]
        assert proof.serialize() == wire.encode_running_proof(0, opp.params, want, [x0])
    assert proof.verify(pp, n, z0, [fe(x)]) is True and proof.verify(pp, n, z0, [fe(x + 1)]) is False
    snark = proof.compress(pp)
    assert snark.verify(pp, n, z0, [fe(x)]) is True and snark.verify(pp, n, z0, [fe(x + 1)]) is False
    for h in (snark, proof, pp):
        h.free()


def test_every_constructor_of_before_makes_the_fq_orientation(ctx):
    from vdf_amd.nova import ro_preset
    t = 5
    made = [public_params(ctx, t), public_params(ctx, t, CIRCUIT_MINROOT_BOUND, flags=1), public_params(ctx, t, CIRCUIT_MINROOT_FORWARD, stencil=0),
            public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, ro=ro_preset(0)), public_params_lanes(ctx, t, 1), public_params_lanes(ctx, t, 2),
            public_params_custom(ctx, CubicFp())]
    for pp in made:
        assert pp.field() == FIELD_FQ
        pp.free()
    both = [public_params(ctx, t, CIRCUIT_MINROOT_FORWARD, field=f) for f in (FIELD_FQ, FIELD_FP)]
    assert [pp.field() for pp in both] == [FIELD_FQ, FIELD_FP] and both[0].digest() == public_params(ctx, t, CIRCUIT_MINROOT_FORWARD).digest()
    for pp in both:
        pp.free()


# ---- 10. the plain-C client -------------------------------------------------------------------------------------------------------------

def test_prove_vesta_client(ctx):
    """examples/prove_vesta (plain C over the two ABIs) as a fresh child process at t = 64 over 3 steps: exit 0, and the digest
    and the SHA-256 of the wire bytes it prints are this host's for the same chain."""
    exe = os.path.join(ROOT, "examples", "prove_vesta")
    assert os.path.exists(exe), "examples/prove_vesta is built by vdf_amd/csrc/Makefile (all)"
    t, n = 64, 3
    # a fresh child process (never an exec of this one)
    r = subprocess.run([exe, "6", str(n), "123", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true" and lines["verify (decoded)"] == "true"
    assert lines["verify with z0 and zi swapped"] == "false" and lines["final state is VestaVDF's"] == "true"
    pp = public_params(ctx, t, CIRCUIT_MINROOT_FORWARD, field=FIELD_FP)
    initial = State.from_ints(FIELD_FP, 123, 0, 0)
    proof, final, _ = NovaVDFProof.eval_and_prove(pp, VestaVDF.new_with_mode(FAST), initial, n)
    assert bytes.fromhex(lines["final state"]) == final.x + final.y + final.i
    assert bytes.fromhex(lines["digest"]) == pp.digest().to_bytes(32, "little")
    snark = proof.compress(pp)
    assert lines["wire sha256"] == hashlib.sha256(snark.serialize()).hexdigest()
    for h in (snark, proof, pp):
        h.free()
