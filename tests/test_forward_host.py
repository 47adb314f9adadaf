"""CPU tests of the forward MinRoot step circuit (include/vdf_nova.h VDF_CIRCUIT_MINROOT_FORWARD) in the host layer of
libvdf_nova.so against its specification, tests/forward_spec.py run through oracle/nova.py's `primary=` seam: shapes and
digests, the augmented circuit's witness, the stencil of the early rows, chains that grow, and soundness of the form.
No device call is made."""
import copy
import json
import os

import numpy as np
import pytest

from oracle import nova as nv, pasta as o
from forward_spec import ForwardMinRootCircuit, chain, oracle_pp
from test_nova_host import c_inputs, st, unmont

import vdf_amd
import vdf_amd.nova as vn
from vdf_amd.minroot import PallasVDF, State

FWD = vn.CIRCUIT_MINROOT_FORWARD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_forward():
    with open(os.path.join(ROOT, "tests", "golden", "forward.json")) as f:
        return json.load(f)


def test_the_kind_is_three_and_the_stencil_code_five():
    assert FWD == 3 and vn.STENCIL_FORWARD == 5


@pytest.mark.parametrize("t", [1, 5, 24])
def test_shape_digest_equals_the_oracle(t):
    """Every triple of A, B, C on both sides hashes to the oracle's `params` for the specification circuit; the shape has
    the size of the bound inverse form and another digest than kinds 0 and 1."""
    pp = oracle_pp(t)
    digest, sizes = vn.shape_digest(t, FWD, 1)
    assert digest == pp.params
    for s in (0, 1):
        sh = pp.shapes[s]
        assert sizes[s] == [sh.num_cons, sh.num_vars, len(sh.A) + len(sh.B) + len(sh.C)]
    d0, s0 = vn.shape_digest(t, 0, 1)
    d1, _ = vn.shape_digest(t, 1, 1)
    assert digest not in (d0, d1)
    assert sizes[0][:2] == s0[0][:2]                       # 3t + 1 variables and 3t + 1 constraints from the step circuit, as BOUND


def test_committed_digests(golden_forward):
    for t in (1, 5):
        assert vn.shape_digest(t, FWD, 1)[0] == int(golden_forward["params"][str(t)], 16)


@pytest.fixture(scope="module")
def oracle_run():
    """Three oracle steps at t = 5 over the forward circuit with every circuit's inputs and outputs recorded."""
    t, n = 5, 3
    rec = []
    orig = nv.synth_fresh

    def spy(pp, side, inp, step):
        fresh, z = orig(pp, side, inp, step)
        rec.append((side, copy.deepcopy(inp), step, fresh, z))
        return fresh, z
    nv.synth_fresh = spy
    try:
        pp = oracle_pp(t, nv.CCommit())
        states = chain(o.State(0x1234, 0, 1), t, n)
        z0 = [states[0].x, states[0].y, states[0].i]
        s = None
        for k in range(n):
            s = nv.prove_step(pp, s, ForwardMinRootCircuit(t, states[k], states[k + 1]), z0)
        assert nv.verify(pp, s, n, z0) == ([states[n].x, states[n].y, states[n].i], [0])
        assert nv.verify(pp, s, n, [states[0].x + 1, states[0].y, states[0].i]) is None      # a wrong z0 is refused
    finally:
        nv.synth_fresh = orig
    return t, pp, rec


def test_augmented_circuit_witness_equals_the_oracle(oracle_run):
    """W, X and z_next of the primary augmented circuit around the forward step: the base step and both later steps."""
    t, pp, rec = oracle_run
    primary = [r for r in rec if r[0] == 0]
    assert len(primary) == 3
    for side, inp, step, fresh, z_next in primary:
        W, X, zn, nc = vn.aug_synthesize(0, t, FWD, c_inputs(0, inp), st(step.result), st(step.input))
        assert nc == pp.shapes[0].num_cons and W.shape[0] == pp.shapes[0].num_vars
        assert unmont(X, o.FIELD_FQ) == fresh.X
        assert unmont(zn, o.FIELD_FQ) == z_next == [step.result.x, step.result.y, step.result.i]
        got = unmont(W, o.FIELD_FQ)
        bad = [k for k in range(len(got)) if got[k] != fresh.W[k]]
        assert not bad, (inp.i, bad[:5])


def test_early_rows_are_the_forward_stencil():
    """shape_stencil reports code 5 with 3t + 1 early rows, and the oracle's own shape has exactly the stencil
    vdf_nifs_cross_term_minroot_forward computes (include/vdf_hip.h) where the host says it is."""
    for t in (1, 2, 3, 7, 64, 100):
        code, row0, nrows, seg = vn.shape_stencil(t, FWD)
        assert code == 5 and nrows == 3 * t + 1
        if t > 7:
            continue
        sh = oracle_pp(t).shapes[0]
        Q, one = o.Q, sh.num_vars
        rows = {k: {} for k in range(3)}
        for k, mat in enumerate((sh.A, sh.B, sh.C)):
            for r, c, v in mat:
                if row0 <= r < row0 + nrows:
                    rows[k].setdefault(r - row0, {})[c] = v % Q
        for j in range(t):
            nx, t1, t2 = seg + 3 * j, seg + 3 * j + 1, seg + 3 * j + 2
            assert rows[0][3 * j] == {nx: 1} == rows[1][3 * j] and rows[2][3 * j] == {t1: 1}
            assert rows[0][3 * j + 1] == {t1: 1} == rows[1][3 * j + 1] and rows[2][3 * j + 1] == {t2: 1}
            assert rows[0][3 * j + 2] == {t2: 1} and rows[1][3 * j + 2] == {nx: 1}
            if j == 0:
                want = {seg - 3: 1, seg - 2: 1}
            else:
                want = {nx - 3: 1, (nx - 6 if j > 1 else seg - 3): 1, seg - 1: 1}
                if j > 1:
                    want[one] = j - 1
            assert rows[2][3 * j + 2] == want
        assert rows[0][3 * t] == {seg + 3 * t: 1} and rows[1][3 * t] == {one: 1} and rows[2][3 * t] == {seg - 1: 1, one: t}
    # the inverse kinds keep their codes
    assert vn.shape_stencil(5, 0)[0] == 3 and vn.shape_stencil(5, 1)[0] == 4


def test_growing_chains_check_what_is_pushed():
    """A trace that does not start at the chain's end and a checkpoint with a wrong counter are refused and append nothing;
    release drops the host trace of a pushed step."""
    t = 8
    v = PallasVDF.new()
    init = State.from_ints(o.FIELD_FQ, 0x77, 0, 3)
    z0, fc = vn.ForwardCircuits.begin(t, init)
    assert z0 == [init.x, init.y, init.i] and len(fc) == 0
    s1, tr1 = v.eval_with_trace(init, t)
    s2, tr2 = v.eval_with_trace(s1, t)
    with pytest.raises(vdf_amd.VdfError):
        fc.push_trace(tr2)                                  # starts at s1, the chain stands at init
    assert len(fc) == 0
    fc.push_trace(tr1)
    assert len(fc) == 1
    res, inp = fc.states(0)
    assert inp == init and res == s1 and res.to_ints(o.FIELD_FQ)[2] == 3 + t
    with pytest.raises(vdf_amd.VdfError):
        fc.push_trace(tr1)                                  # the same step twice
    cps = v.eval_checkpoints(s1, t, 4)
    assert cps[-1] == s2
    bad = list(cps)
    bad[1] = State(bad[1].x, bad[1].y, State.from_ints(o.FIELD_FQ, 0, 0, 3 + t + 5).i)
    with pytest.raises(vdf_amd.VdfError):
        fc.push_checkpoints(4, bad)
    with pytest.raises(vdf_amd.VdfError):
        fc.push_checkpoints(4, v.eval_checkpoints(init, t, 4))        # states[0] is not the chain's end
    with pytest.raises(vdf_amd.VdfError):
        fc.push_checkpoints(3, cps)                          # 3 does not divide 8
    assert len(fc) == 1
    fc.push_checkpoints(4, cps)
    assert len(fc) == 2 and fc.states(1) == (s2, s1)
    fc.push_trace(v.eval_with_trace(s2, t)[1])
    assert fc.host_bytes() == 2 * 2 * (t + 1) * 32 + 3 * 96
    fc.release(0, 1)
    assert fc.host_bytes() == 2 * (t + 1) * 32 + 3 * 96
    fc.release(0, 3)
    assert fc.host_bytes() == 3 * 96 and fc.memory() == (0, 0)
    fc.free()
    # the push entry points are for forward chains only
    z0i, inv = vn.InverseMinRootCircuit.eval_and_make_circuits(v, t, 1, init)
    alias = vn.ForwardCircuits(inv.handle, t)
    try:
        with pytest.raises(vdf_amd.VdfError):
            alias.push_trace(tr1)
    finally:
        alias.handle = None                                  # `inv` owns the handle
    inv.free()


def test_every_round_variable_is_bound():
    """Soundness on the oracle's CS: the step circuit alone, satisfied by the honest witness, is violated by a change to ANY
    x_(j+1) -- the form has no counterpart of the free new_x of the reference's circuit (tests/test_oracle_nova.py)."""
    t = 6
    s0 = o.State(0xABCDEF, 0x1234, 7)
    s1 = o.minroot_eval(s0, t, o.FIELD_FQ)
    cs = nv.CS(o.FIELD_FQ)
    z = [cs.alloc_io(v) for v in (s0.x, s0.y, s0.i)]
    out = ForwardMinRootCircuit(t, s0, s1).synthesize(cs, z)
    assert [n.v for n in out] == [s1.x, s1.y, s1.i]
    sh = cs.shape()
    assert sh.num_vars == 3 * t + 1 == sh.num_cons
    E = [0] * sh.num_cons
    assert o.is_sat_relaxed(sh, cs.W, E, 1, cs.X, o.Q)
    for j in range(t):
        for delta in (1, o.Q - 1, 0x5555):
            W = list(cs.W)
            W[3 * j] = (W[3 * j] + delta) % o.Q
            assert not o.is_sat_relaxed(sh, W, E, 1, cs.X, o.Q), j
            # ... also when the prover recomputes the powers that depend on it: the product must still be x_j + y_j
            W[3 * j + 1] = W[3 * j] ** 2 % o.Q
            W[3 * j + 2] = W[3 * j + 1] ** 2 % o.Q
            assert not o.is_sat_relaxed(sh, W, E, 1, cs.X, o.Q), j
    # every variable of the circuit is in some constraint with a non-zero coefficient, and the only variable of a round
    # that no earlier one determines is the fifth root, which x -> x^5 (a bijection on Fq: gcd(5, q - 1) = 1) pins
    used = {c for mat in (sh.A, sh.B, sh.C) for _, c, v in mat if v % o.Q}
    assert set(range(sh.num_vars)) <= used and (o.Q - 1) % 5 != 0
