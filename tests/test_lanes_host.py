"""CPU tests of the forward MinRoot step circuit in lanes (include/vdf_nova.h VDF_CIRCUIT_MINROOT_FORWARD_LANES) in the host
layer of libvdf_nova.so against its specification, tests/lanes_spec.py run through oracle/nova.py's `primary=` seam: shapes
and digests, what a lane costs, the augmented circuit's witness, the stencil of the early rows lane by lane, chains that grow
in lanes, and soundness of the form.  No device call is made."""
import copy
import json
import os

import numpy as np
import pytest

from oracle import nova as nv, pasta as o
from lanes_spec import LanesForwardCircuit, chains, flat, oracle_pp
from test_nova_host import c_inputs, mont, st, unmont

import vdf_amd
import vdf_amd.nova as vn
from vdf_amd.minroot import PallasVDF, State

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_lanes():
    with open(os.path.join(ROOT, "tests", "golden", "lanes.json")) as f:
        return json.load(f)


def test_the_kind_is_four_the_stencil_code_six_and_the_cap_sixteen():
    assert vn.CIRCUIT_MINROOT_FORWARD_LANES == 4 and vn.STENCIL_FORWARD_LANES == 6 and vn.MAX_LANES == 16
    for lanes in (0, 17):
        with pytest.raises(vdf_amd.VdfError):
            vn.shape_digest_lanes(3, lanes, 1)
        with pytest.raises(vdf_amd.VdfError):
            vn.shape_stencil_lanes(3, lanes)


@pytest.mark.parametrize("L,t", [(2, 1), (2, 3), (4, 2), (3, 5)])
def test_shape_digest_equals_the_oracle(L, t):
    """Every triple of A, B, C on both sides hashes to the oracle's `params` for the specification circuit."""
    pp = oracle_pp(t, L)
    digest, sizes = vn.shape_digest_lanes(t, L, 1)
    assert digest == pp.params
    for s in (0, 1):
        sh = pp.shapes[s]
        assert sizes[s] == [sh.num_cons, sh.num_vars, len(sh.A) + len(sh.B) + len(sh.C)]
    assert vn.shape_digest_lanes(t, L, 0)[0] != digest          # the generator family is part of the digest


def test_committed_digests(golden_lanes):
    for key, want in golden_lanes["params"].items():
        L, t = (int(v) for v in key.split(","))
        assert vn.shape_digest_lanes(t, L, 1)[0] == int(want, 16)


def test_one_lane_is_the_forward_circuit():
    for t in (1, 5):
        assert vn.shape_digest_lanes(t, 1, 1) == vn.shape_digest(t, vn.CIRCUIT_MINROOT_FORWARD, 1)
        assert vn.shape_stencil_lanes(t, 1) == vn.shape_stencil(t, vn.CIRCUIT_MINROOT_FORWARD)
        assert vn.shape_stencil_lanes(t, 1)[0] == vn.STENCIL_FORWARD


@pytest.mark.parametrize("t", [2, 5])
def test_what_a_lane_costs(t):
    """The primary side's size is one lane's plus 3t + 1 rounds' worth per extra lane plus a remainder per extra lane -- the
    longer z0 / zi the two state hashes absorb -- which is the same for every extra lane and does not depend on t; the
    secondary side does not grow."""
    sizes = {L: vn.shape_digest_lanes(t, L, 1)[1] for L in (1, 2, 3, 4, 16)}
    rem = []
    for L in (2, 3, 4):
        rem.append(tuple(sizes[L][0][k] - sizes[L - 1][0][k] - (3 * t + 1) for k in (0, 1)))
        assert sizes[L][1] == sizes[1][1]
    print("t = %d: constraints, variables per extra lane outside the rounds: %s" % (t, rem))
    assert rem[0] == rem[1] == rem[2]
    assert tuple(sizes[16][0][k] - sizes[1][0][k] - 15 * (3 * t + 1) for k in (0, 1)) == tuple(15 * r for r in rem[0])
    assert 1000 < rem[0][0] < 1100                          # about 1,059: four permutations of the random oracle


@pytest.fixture(scope="module")
def oracle_run():
    """Three oracle steps at L = 2, t = 3 with every circuit's inputs and outputs recorded."""
    L, t, n = 2, 3, 3
    rec = []
    orig = nv.synth_fresh

    def spy(pp, side, inp, step):
        fresh, z = orig(pp, side, inp, step)
        rec.append((side, copy.deepcopy(inp), step, fresh, z))
        return fresh, z
    nv.synth_fresh = spy
    try:
        pp = oracle_pp(t, L, nv.CCommit())
        states = chains([o.State(0x1234, 0, 1), o.State(0x5678, 9, 1000)], t, n)
        z0 = flat(states[0])
        s = None
        for k in range(n):
            s = nv.prove_step(pp, s, LanesForwardCircuit(t, states[k], states[k + 1]), z0)
    finally:
        nv.synth_fresh = orig
    return L, t, n, pp, rec, states, s


def test_augmented_circuit_witness_equals_the_oracle(oracle_run):
    """W, X and z_next of the primary augmented circuit around the lanes step: the base step and both later steps."""
    L, t, n, pp, rec, states, _ = oracle_run
    primary = [r for r in rec if r[0] == 0]
    assert len(primary) == n
    for side, inp, step, fresh, z_next in primary:
        short = copy.copy(inp)
        short.z0, short.zi = inp.z0[:3], inp.zi[:3]          # the struct's own z0 / zi are not read: the arrays are
        z0, zi = (list(mont(v, o.FIELD_FQ)[k].tobytes() for k in range(3 * L)) for v in (inp.z0, inp.zi))
        W, X, zn, nc = vn.aug_synthesize_lanes(t, L, c_inputs(0, short), z0, zi, [st(s) for s in step.results], [st(s) for s in step.inputs])
        assert nc == pp.shapes[0].num_cons and W.shape[0] == pp.shapes[0].num_vars
        assert unmont(X, o.FIELD_FQ) == fresh.X
        assert unmont(zn, o.FIELD_FQ) == z_next == flat(step.results)
        got = unmont(W, o.FIELD_FQ)
        bad = [k for k in range(len(got)) if got[k] != fresh.W[k]]
        assert not bad, (inp.i, bad[:5])


def test_a_proof_of_swapped_lanes_is_another_statement(oracle_run):
    """verify hands back the lanes' outputs in the lanes' order: the outputs of two lanes swapped are not what it returns, and a
    z0 changed in lane 1 only is refused."""
    L, t, n, pp, rec, states, s = oracle_run
    z0 = flat(states[0])
    got = nv.verify(pp, s, n, z0)
    assert got == (flat(states[n]), [0])
    assert got[0] != flat(states[n][::-1])
    bad = list(z0)
    bad[3] += 1
    assert nv.verify(pp, s, n, bad) is None
    assert nv.verify(pp, s, n, flat(states[0][::-1])) is None


@pytest.mark.parametrize("L", [2, 3])
def test_early_rows_are_the_stencil_lane_by_lane(L):
    """shape_stencil_lanes reports code 6 with L (3t + 1) early rows as ONE run, the lanes' variables lane-major from seg_begin
    and the 3L inputs right in front of them; and for t <= 7 the oracle's own shape has, lane by lane, exactly the stencil
    vdf_nifs_cross_term_minroot_forward_lanes computes (include/vdf_hip.h) -- each lane's j = 0 and j = 1 rows reading ITS inputs."""
    for t in (1, 2, 3, 7, 64):
        code, row0, nrows, seg0 = vn.shape_stencil_lanes(t, L)
        per = 3 * t + 1
        assert code == 6 and nrows == L * per
        if t > 7:
            continue
        sh = oracle_pp(t, L).shapes[0]
        Q, one = o.Q, sh.num_vars
        rows = {k: {} for k in range(3)}
        for k, mat in enumerate((sh.A, sh.B, sh.C)):
            for r, c, v in mat:
                if row0 <= r < row0 + nrows:
                    rows[k].setdefault(r - row0, {})[c] = v % Q
        for l in range(L):
            seg, zin, rb = seg0 + l * per, seg0 - 3 * L + 3 * l, l * per
            for j in range(t):
                nx, t1, t2 = seg + 3 * j, seg + 3 * j + 1, seg + 3 * j + 2
                r = rb + 3 * j
                assert rows[0][r] == {nx: 1} == rows[1][r] and rows[2][r] == {t1: 1}
                assert rows[0][r + 1] == {t1: 1} == rows[1][r + 1] and rows[2][r + 1] == {t2: 1}
                assert rows[0][r + 2] == {t2: 1} and rows[1][r + 2] == {nx: 1}
                if j == 0:
                    want = {zin: 1, zin + 1: 1}
                else:
                    want = {nx - 3: 1, (nx - 6 if j > 1 else zin): 1, zin + 2: 1}
                    if j > 1:
                        want[one] = j - 1
                assert rows[2][r + 2] == want, (l, j)
            r = rb + 3 * t
            assert rows[0][r] == {seg + 3 * t: 1} and rows[1][r] == {one: 1} and rows[2][r] == {zin + 2: 1, one: t}


def test_growing_chains_check_every_lane():
    """A trace or a checkpoint set that is wrong in lane 1 only is refused, names the lane and appends nothing; the single-lane
    pushes are refused on a chain of two lanes; host bytes are accounted per lane; a lanes chain of one lane is a forward chain."""
    t, L = 8, 2
    v = PallasVDF.new()
    inits = [State.from_ints(o.FIELD_FQ, 0x77, 0, 3), State.from_ints(o.FIELD_FQ, 0x99, 5, 100)]
    z0, lc = vn.LaneCircuits.begin(t, inits)
    assert z0 == [e for s in inits for e in (s.x, s.y, s.i)] and len(lc) == 0
    assert vn.nova_lib.vdf_nova_circuits_lanes(lc.handle) == 2
    s1, tr1 = zip(*[v.eval_with_trace(s, t) for s in inits])
    s2, tr2 = zip(*[v.eval_with_trace(s, t) for s in s1])
    with pytest.raises(vdf_amd.VdfError) as e:
        lc.push_traces([tr1[0], tr2[1]])                    # lane 1 starts at its next step
    assert "lane 1" in str(e.value) and len(lc) == 0
    with pytest.raises(vdf_amd.VdfError):
        lc.push_traces([tr1[1], tr1[0]])                    # the lanes swapped: lane 0 is named first
    single = vn.ForwardCircuits(lc.handle, t)
    try:
        with pytest.raises(vdf_amd.VdfError):
            single.push_trace(tr1[0])
        with pytest.raises(vdf_amd.VdfError):
            single.push_checkpoints(4, v.eval_checkpoints(inits[0], t, 4))
    finally:
        single.handle = None                                # `lc` owns the handle
    assert len(lc) == 0
    # a stride wider than the traces
    wide = np.zeros((L, 2 * (t + 3), 4), dtype="<u8")
    for l in range(L):
        wide[l, :2 * (t + 1)] = np.asarray(tr1[l]).reshape(-1, 4)
    lc.push_traces(wide, lane_stride=t + 3)
    assert len(lc) == 1
    for l in range(L):
        assert lc.lane_states(0, l) == (s1[l], inits[l])
    assert lc.states(0) == (s1[0], inits[0])
    with pytest.raises(vdf_amd.VdfError):
        lc.lane_states(0, 2)
    cps = [v.eval_checkpoints(s, t, 4) for s in s1]
    assert [c[-1] for c in cps] == list(s2)
    bad = [list(c) for c in cps]
    bad[1][1] = State(bad[1][1].x, bad[1][1].y, State.from_ints(o.FIELD_FQ, 0, 0, 1).i)
    with pytest.raises(vdf_amd.VdfError) as e:
        lc.push_checkpoints(4, bad)
    assert "lane 1" in str(e.value)
    with pytest.raises(vdf_amd.VdfError) as e:
        lc.push_checkpoints(4, [cps[0], v.eval_checkpoints(inits[1], t, 4)])   # lane 1 does not start at its end
    assert "lane 1" in str(e.value)
    with pytest.raises(vdf_amd.VdfError):
        lc.push_checkpoints(3, cps)                          # 3 does not divide 8
    assert len(lc) == 1
    lc.push_checkpoints(4, cps)
    assert len(lc) == 2 and lc.lane_states(1, 1) == (s2[1], s1[1])
    assert lc.host_bytes() == L * 2 * (t + 1) * 32 + L * 3 * 96
    lc.release(0, 1)
    assert lc.host_bytes() == L * 3 * 96 and lc.memory() == (0, 0)
    lc.free()
    # one lane IS a forward chain: the single-lane calls work on it, and the lanes calls too
    z0, one = vn.LaneCircuits.begin(t, inits[:1])
    assert z0 == [inits[0].x, inits[0].y, inits[0].i]
    fwd = vn.ForwardCircuits(one.handle, t)
    try:
        fwd.push_trace(tr1[0])
        one.push_traces([tr2[0]])
        assert len(one) == 2 and fwd.states(1) == (s2[0], s1[0]) and one.lane_states(1, 0) == (s2[0], s1[0])
    finally:
        fwd.handle = None
    one.free()
    for lanes in (0, 17):
        with pytest.raises(vdf_amd.VdfError):
            vn.LaneCircuits.begin(t, [inits[0]] * lanes)


@pytest.mark.parametrize("every", [None, 2, 4])
def test_a_forward_chain_and_a_chain_of_one_lane_are_the_same_chain(every):
    """Two steps at t = 4 pushed through the single-lane calls and through the lanes calls with one lane -- as traces
    (every = None) or as checkpoints every 2 and every 4 rounds: the same z0, the same states and lane-0 states of every step,
    and no lane 1 on either."""
    t, n = 4, 2
    v = PallasVDF.new()
    init = State.from_ints(o.FIELD_FQ, 0x4321, 0, 11)
    z0f, fc = vn.ForwardCircuits.begin(t, init)
    z0l, lc = vn.LaneCircuits.begin(t, [init])
    assert z0f == z0l == [init.x, init.y, init.i]
    want, s = [], init
    for _ in range(n):
        if every is None:
            nxt, tr = v.eval_with_trace(s, t)
            fc.push_trace(tr)
            lc.push_traces([tr])
        else:
            cps = v.eval_checkpoints(s, t, every)
            nxt = cps[-1]
            fc.push_checkpoints(every, cps)
            lc.push_checkpoints(every, [cps])
        want.append((nxt, s))
        s = nxt
    assert len(fc) == len(lc) == n and fc.host_bytes() == lc.host_bytes()
    lane_states = vn.LaneCircuits.lane_states                # (ForwardCircuits has no method for it: the call is the handle's)
    for k in range(n):
        assert fc.states(k) == lc.states(k) == want[k]
        assert lane_states(fc, k, 0) == lane_states(lc, k, 0) == want[k]
        for c in (fc, lc):
            with pytest.raises(vdf_amd.VdfError):
                lane_states(c, k, 1)
    fc.free(); lc.free()


def test_every_root_of_every_lane_is_bound():
    """Soundness on the oracle's CS at L = 3, t = 4: the step circuit alone, satisfied by the honest witness, is violated by a
    change to ANY x_(j+1) of ANY lane, also when the prover recomputes the powers that depend on it."""
    L, t = 3, 4
    s0 = [o.State(0xABCDEF + l, 0x1234 * l, 7 + 100 * l) for l in range(L)]
    s1 = [o.minroot_eval(s, t, o.FIELD_FQ) for s in s0]
    cs = nv.CS(o.FIELD_FQ)
    z = [cs.alloc_io(v) for v in flat(s0)]
    out = LanesForwardCircuit(t, s0, s1).synthesize(cs, z)
    assert [n.v for n in out] == flat(s1)
    sh = cs.shape()
    per = 3 * t + 1
    assert sh.num_vars == L * per == sh.num_cons
    E = [0] * sh.num_cons
    assert o.is_sat_relaxed(sh, cs.W, E, 1, cs.X, o.Q)
    for l in range(L):
        for j in range(t):
            for delta in (1, o.Q - 1, 0x5555):
                W = list(cs.W)
                at = l * per + 3 * j
                W[at] = (W[at] + delta) % o.Q
                assert not o.is_sat_relaxed(sh, W, E, 1, cs.X, o.Q), (l, j)
                W[at + 1] = W[at] ** 2 % o.Q
                W[at + 2] = W[at + 1] ** 2 % o.Q
                assert not o.is_sat_relaxed(sh, W, E, 1, cs.X, o.Q), (l, j)
    used = {c for mat in (sh.A, sh.B, sh.C) for _, c, v in mat if v % o.Q}
    assert set(range(sh.num_vars)) <= used
