"""CPU tests of the cycle in the other orientation (include/vdf_nova.h vdf_nova_public_params_field: the primary circuit over
Fp, G1 = Vesta, the chains of VestaVDF) in the host layer of libvdf_nova.so against oracle/nova.py with its two orientation
tuples exchanged (tests/vesta_spec.py): shapes and digests, the triples, both augmented circuits' witnesses, the stencil
codes, and circuits handles that remember their field.  No device call is made."""
import copy
import json
import os

import numpy as np
import pytest

from oracle import nova as nv, pasta as o
import vesta_spec as vs
from test_nova_host import c_inputs, st, unmont

import vdf_amd
import vdf_amd.nova as vn
from vdf_amd.minroot import PallasVDF, VestaVDF, State

FP, FQ = o.FIELD_FP, o.FIELD_FQ
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_vesta():
    with open(os.path.join(ROOT, "tests", "golden", "vesta.json")) as f:
        return json.load(f)


def test_the_field_constants_are_the_oracles():
    assert (vn.FIELD_FP, vn.FIELD_FQ) == (FP, FQ) and VestaVDF.FIELD == FP and PallasVDF.FIELD == FQ


@pytest.mark.parametrize("kind,t,lanes", [(vs.FORWARD, 1, 1), (vs.FORWARD, 5, 1), (vs.FORWARD, 24, 1), (vs.BOUND, 5, 1), (vs.REFERENCE, 5, 1),
                                          (vs.LANES, 5, 1), (vs.LANES, 5, 2), (vs.LANES, 5, 3)])
def test_shape_digest_equals_the_swapped_oracle(kind, t, lanes):
    """Every triple of A, B, C on both sides hashes to the swapped oracle's `params`; the sizes are the oracle's; the digest is
    not the one of the same (t, kind) over Fq although the formula has no orientation byte: the matrices differ."""
    with vs.swapped():
        pp = vs.oracle_pp(FP, kind, t, lanes)
    digest, sizes = vn.shape_digest_field(FP, t, kind, lanes, 1)
    assert digest == pp.params
    for s in (0, 1):
        sh = pp.shapes[s]
        assert sizes[s] == [sh.num_cons, sh.num_vars, len(sh.A) + len(sh.B) + len(sh.C)]
    dq, sq = vn.shape_digest_field(FQ, t, kind, lanes, 1)
    assert dq != digest and [s[:2] for s in sq] == [s[:2] for s in sizes]
    # FQ through the general form is what the entry points of before give
    want = vn.shape_digest_lanes(t, lanes, 1) if kind == vs.LANES else vn.shape_digest(t, kind, 1)
    assert (dq, sq) == want


def test_committed_digests(golden_vesta):
    for name, (kind, lanes) in {"bound": (vs.BOUND, 1), "reference": (vs.REFERENCE, 1), "forward": (vs.FORWARD, 1),
                                "forward_lanes_2": (vs.LANES, 2)}.items():
        for t in (1, 5):
            assert vn.shape_digest_field(FP, t, kind, lanes, 1)[0] == int(golden_vesta["params"][name][str(t)], 16), (name, t)


def test_general_forms_refuse_what_they_cannot_build():
    for bad in (lambda: vn.shape_digest_field(2, 5, vs.FORWARD), lambda: vn.shape_digest_field(FP, 5, vs.FORWARD, 2),
                lambda: vn.shape_digest_field(FP, 5, vs.LANES, 0), lambda: vn.shape_digest_field(FP, 5, vs.LANES, vn.MAX_LANES + 1),
                lambda: vn.shape_digest_field(FP, 5, 2), lambda: vn.shape_stencil_field(FP, 5, vs.BOUND, 2),
                lambda: vn.shape_export_field(-1, 5, vs.FORWARD)):
        with pytest.raises(vdf_amd.VdfError) as e:
            bad()
        assert e.value.code == 1


@pytest.mark.parametrize("kind,lanes", [(vs.FORWARD, 1), (vs.REFERENCE, 1), (vs.LANES, 2)])
def test_shape_export_equals_the_oracle_shape_on_both_sides(kind, lanes):
    t = 5
    with vs.swapped():
        pp = vs.oracle_pp(FP, kind, t, lanes)
    for side, field in ((0, FP), (1, FQ)):
        m = o.modulus(field)
        sh = pp.shapes[side]
        mats = vn.shape_export_field(FP, t, kind, lanes, side)
        for (rows, cols, vals), want in zip(mats, (sh.A, sh.B, sh.C)):
            got = list(zip(rows.tolist(), cols.tolist(), unmont(vals, field)))
            assert got == [(r, c, v % m) for r, c, v in want]


@pytest.fixture(scope="module")
def oracle_run():
    """Three swapped-oracle steps at t = 5 over the forward circuit over Fp, every circuit's inputs and outputs recorded; the
    oracle's tuples are back in place when the fixture returns."""
    t, n = 5, 3
    rec = []
    orig = nv.synth_fresh

    def spy(pp, side, inp, step):
        fresh, z = orig(pp, side, inp, step)
        rec.append((side, copy.deepcopy(inp), step, fresh, z))
        return fresh, z
    with vs.swapped():
        nv.synth_fresh = spy
        try:
            pp = vs.oracle_pp(FP, vs.FORWARD, t, commit=nv.CCommit())
            states = vs.chain(FP, o.State(0x1234, 0, 1), t, n)
            z0 = [states[0].x, states[0].y, states[0].i]
            s = None
            for k in range(n):
                s = nv.prove_step(pp, s, vs.ForwardMinRootCircuit(FP, t, states[k], states[k + 1]), z0)
            assert nv.verify(pp, s, n, z0) == ([states[n].x, states[n].y, states[n].i], [0])
            assert nv.verify(pp, s, n, [states[0].x + 1, states[0].y, states[0].i]) is None
        finally:
            nv.synth_fresh = orig
    assert nv.SIDE_FIELD == (FQ, FP) and nv.SIDE_CURVE == (o.CURVE_PALLAS, o.CURVE_VESTA)
    return t, pp, rec


def test_both_augmented_circuits_equal_the_oracle_on_every_variable(oracle_run):
    """W, X and z_next of the primary circuit (over Fp, around the forward step) and of the secondary circuit (over Fq, around
    TrivialTestCircuit) for the base step and both later steps."""
    t, pp, rec = oracle_run
    assert [r[0] for r in rec] == [0, 1] * 3
    for side, inp, step, fresh, z_next in rec:
        field = FP if side == 0 else FQ
        with vs.swapped():
            a = c_inputs(side, inp)                  # (reads the oracle's tuples for the fields of the two sides)
        if side == 0:
            W, X, zn, nc = vn.aug_synthesize_field(FP, 0, t, vs.FORWARD, a, [st(step.result, FP)], [st(step.input, FP)])
            assert z_next == [step.result.x, step.result.y, step.result.i]
        else:
            W, X, zn, nc = vn.aug_synthesize_field(FP, 1, t, vs.FORWARD, a)
        assert nc == pp.shapes[side].num_cons and W.shape[0] == pp.shapes[side].num_vars
        assert unmont(X, field) == fresh.X
        assert unmont(zn, field) == z_next
        got = unmont(W, field)
        bad = [k for k in range(len(got)) if got[k] != fresh.W[k]]
        assert not bad, (side, inp.i, bad[:5])


def test_lanes_augmented_circuit_equals_the_oracle():
    """The primary circuit around two lanes over Fp at the base step: z0 / zi from the arrays, one state per lane."""
    t, L = 3, 2
    with vs.swapped():
        pp = vs.oracle_pp(FP, vs.LANES, t, L, commit=nv.CCommit())
        sts = vs.chains(FP, [o.State(5, 0, 0), o.State(6, 1, 9)], t, 1)
        z0 = vs.flat(sts[0])
        inp = nv.dummy_inputs(3 * L)
        inp.params, inp.z0, inp.zi = pp.params, list(z0), list(z0)
        fresh, z_next = nv.synth_fresh(pp, 0, inp, vs.LanesForwardCircuit(FP, t, sts[0], sts[1]))
        small = copy.deepcopy(inp)
        small.z0, small.zi = small.z0[:3], small.zi[:3]
        a = c_inputs(0, small)
    from test_nova_host import mont
    z0b = [bytes(r) for r in mont(z0, FP).view(np.uint8).reshape(-1, 32)]
    W, X, zn, nc = vn.aug_synthesize_field(FP, 0, t, vs.LANES, a, [st(s, FP) for s in sts[1]], [st(s, FP) for s in sts[0]], z0=z0b, zi=z0b, lanes=L)
    assert nc == pp.shapes[0].num_cons and unmont(W, FP) == fresh.W and unmont(X, FP) == fresh.X
    assert unmont(zn, FP) == z_next == vs.flat(sts[1])


@pytest.mark.parametrize("t", [1, 5, 1024])
def test_stencil_codes_are_those_of_the_other_orientation(t):
    """5 / 6 / 4 / 3 with the same early rows and segment as over Fq: the detection compares with constants of the right field."""
    for kind, lanes, code in ((vs.FORWARD, 1, 5), (vs.LANES, 2, 6), (vs.REFERENCE, 1, 4), (vs.BOUND, 1, 3)):
        got = vn.shape_stencil_field(FP, t, kind, lanes)
        assert got[0] == code and got[2] == lanes * (3 * t + 1)
        want = vn.shape_stencil_lanes(t, lanes) if kind == vs.LANES else vn.shape_stencil(t, kind)
        assert got == want == vn.shape_stencil_field(FQ, t, kind, lanes)


def test_circuits_remember_their_field_and_check_with_it():
    """forward_begin_field(FP) takes a VestaVDF chain by traces and by checkpoints and refuses the PallasVDF trace from the same
    start (its first round already differs); from_checkpoints_field checks .i over Fp."""
    t = 8
    v, w = VestaVDF.new(), PallasVDF.new()
    init = State.from_ints(FP, 0x77, 0, 3)
    z0, fc = vn.ForwardCircuits.begin(t, init, field=FP)
    assert fc.field() == FP and z0 == [init.x, init.y, init.i]
    s1, tr1 = v.eval_with_trace(init, t)
    _, tr1q = w.eval_with_trace(State.from_ints(FQ, 0x77, 0, 3), t)
    # the same integers are other Montgomery bytes in the other field: compare the chains as integers
    assert State(*[bytes(r) for r in tr1q[2:4].view(np.uint8).reshape(2, 32)], init.i).to_ints(FQ)[:2] != \
        State(*[bytes(r) for r in tr1[2:4].view(np.uint8).reshape(2, 32)], init.i).to_ints(FP)[:2]
    with pytest.raises(vdf_amd.VdfError) as e:
        fc.push_trace(tr1q)
    assert e.value.code == 1 and len(fc) == 0
    fc.push_trace(tr1)
    res, inp = fc.states(0)
    assert inp == init and res == s1 and res.to_ints(FP)[2] == 3 + t
    cps = v.eval_checkpoints(s1, t, 4)
    bad = list(cps)
    bad[1] = State(bad[1].x, bad[1].y, State.from_ints(FQ, 0, 0, 3 + t + 4).i)      # the right counter in the WRONG field's form
    with pytest.raises(vdf_amd.VdfError):
        fc.push_checkpoints(4, bad)
    fc.push_checkpoints(4, cps)
    assert len(fc) == 2 and fc.states(1) == (cps[-1], s1)
    fc.free()
    # a counter that wraps round p: i = p - 2 counts on to 2 over Fp (over Fq it would be p + 2)
    hi = State.from_ints(FP, 9, 1, o.P - 2)
    cps = v.eval_checkpoints(hi, 2 * t, 4)
    assert cps[-1].to_ints(FP)[2] == (o.P - 2 + 2 * t) % o.P
    z0c, cc = vn.InverseMinRootCircuit.from_checkpoints(t, 4, 2, cps, field=FP)
    assert cc.field() == FP and len(cc) == 2 and z0c == [cps[-1].x, cps[-1].y, cps[-1].i]
    cc.free()
    with pytest.raises(vdf_amd.VdfError) as e:
        vn.InverseMinRootCircuit.from_checkpoints(t, 4, 2, cps, field=FQ)
    assert e.value.code == 1
    # eval_and_make_circuits takes the field from the VDF
    z0e, ec = vn.InverseMinRootCircuit.eval_and_make_circuits(v, t, 2, init)
    assert ec.field() == FP and ec.states(1) == (s1, init)
    assert z0e == [x for x in (lambda s: (s.x, s.y, s.i))(v.eval(init, 2 * t))]
    ec.free()
    z0l, lc = vn.LaneCircuits.begin(t, [init, hi], field=FP)
    assert lc.field() == FP
    lc.push_traces([tr1, v.eval_with_trace(hi, t)[1]])
    assert lc.lane_states(0, 1)[0].to_ints(FP)[2] == (o.P - 2 + t) % o.P
    lc.free()


def test_every_constructor_of_before_is_fq():
    t = 4
    v = PallasVDF.new()
    init = State.from_ints(FQ, 1, 2, 3)
    made = [vn.InverseMinRootCircuit.eval_and_make_circuits(v, t, 1, init)[1], vn.ForwardCircuits.begin(t, init)[1],
            vn.LaneCircuits.begin(t, [init, init])[1], vn.InverseMinRootCircuit.from_checkpoints(t, 2, 1, v.eval_checkpoints(init, t, 2))[1]]
    for c in made:
        assert c.field() == FQ
        c.free()
    assert vn.nova_lib.vdf_nova_circuits_field(None) == -1 and vn.nova_lib.vdf_nova_pp_field(None) == -1
