"""GPU: the batch verifier of compressed proofs with every proof's M(r_x, r_y) evaluated in passes over the shape
(vdf_nova_pp_set_verify_multi; vdf_sparse_eval_multi under it).  The switch changes how the value is computed, never a verdict:
for n = 0 (each replay's own device sequence, the single verifier's), 1, 2 and 16 points per pass, ok[] is the same list for valid
batches, for tampers that the deferred comparison catches (w_eval on either side, the last inner-round element), for one that
only the combined group check catches (an opening's sent vector), for a wrong step count and for a permuted batch.  The counters
say how many passes ran and how many points failed, so no case passes by running the other path."""
import numpy as np
import pytest

from oracle import pasta as o
from vdf_amd.hip import VdfError
from vdf_amd.minroot import EvalMode, PallasVDF, VestaVDF, State, FIELD_FP, FIELD_FQ
from vdf_amd.nova import (CompressedNovaVDFProof, InverseMinRootCircuit, LaneCircuits, NovaVDFProof, CIRCUIT_MINROOT_REFERENCE,
                          public_params, public_params_lanes, verify_compressed_batch)

pytestmark = pytest.mark.gpu
T, STEPS = 16, 2
MODES = [0, 1, 2, 16]
FAST = EvalMode.LTRAddChainSequential


def _zvec(s):
    return [s.x, s.y, s.i]


def _sections(pp, side):
    """Byte offsets in the flat encoding (to_bytes) of side `side`'s argument: 3 s outer elements, 4 claims, 2 l1 inner elements,
    w_eval, then the two openings (L, R per round, then the sent vector of 16)."""
    base = 0
    for sd in range(side + 1):
        sz = pp.sizes(sd)
        s = (sz["num_cons"] - 1).bit_length()
        l1 = (sz["num_vars"] - 1).bit_length() + 1
        kW, kE = (l1 - 1) - 4, s - 4
        head = base + 32 * (3 * s + 4 + 2 * l1 + 1)
        sect = {"inner.last": base + 32 * (3 * s + 4 + 2 * l1 - 1), "w_eval": base + 32 * (3 * s + 4 + 2 * l1), "ipaW.a0": head + 128 * kW}
        base += 32 * (3 * s + 4 + 2 * l1 + 1 + 16 + 16) + 128 * (kW + kE)
    return sect


def _tampered(pp, item, place, side, field=FIELD_FQ):
    """a copy of the entry with one element of its argument raised by one"""
    m = o.modulus(field if side == 0 else 1 - field)                          # side 0's scalars are the chain's field
    bad = CompressedNovaVDFProof.deserialize(pp, item[0].serialize())
    data = bytearray(bad.to_bytes())
    off = _sections(pp, side)[place]
    data[off:off + 32] = ((int.from_bytes(data[off:off + 32], "little") + 1) % m).to_bytes(32, "little")
    bad.set_bytes(bytes(data))
    return (bad,) + tuple(item[1:])


def _under_every_mode(pp, batch, want):
    """the verdicts under n = 0, 1, 2, 16 -- all the same list; returns the counters' change per mode"""
    deltas = {}
    for n in MODES:
        pp.set_verify_multi(n)
        assert pp.verify_multi == n
        before = pp.verify_multi_stats()
        got = verify_compressed_batch(pp, batch)
        after = pp.verify_multi_stats()
        assert got == want, (n, got)
        deltas[n] = tuple(a - b for a, b in zip(after, before))
    assert deltas[0] == (0, 0, 0)                                             # the per-proof sequence launches no pass
    return deltas


@pytest.fixture(scope="module")
def six(ctx):
    pp = public_params(ctx, T, CIRCUIT_MINROOT_REFERENCE)
    initial_mode = pp.verify_multi
    items = []
    for k in range(6):
        x = o.rand_fe(700 + k, 0, o.Q)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), T, STEPS, State.from_ints(FIELD_FQ, x, 0, 1))
        snark = NovaVDFProof.prove_recursively(pp, circuits, T, z0).compress(pp)
        items.append((snark, STEPS, z0, _zvec(State.from_ints(FIELD_FQ, x, 0, 1))))
    wires = [it[0].serialize() for it in items]
    assert len(set(wires)) == 6
    yield pp, items
    assert [it[0].serialize() for it in items] == wires                       # verification leaves every proof as it was
    pp.set_verify_multi(initial_mode)


def test_all_valid(six):
    pp, items = six
    d = _under_every_mode(pp, items, [True] * 6)
    # six live entries on each of the two sides: 6 + 6 passes of one point, 3 + 3 of two, 1 + 1 of six
    assert d[1] == (12, 12, 0) and d[2] == (6, 12, 0) and d[16] == (2, 12, 0)
    assert all(it[0].verify(pp, *it[1:]) for it in items[:2])


@pytest.mark.parametrize("side", [0, 1])
def test_w_eval_tamper_fails_one_point(six, side):
    pp, items = six
    batch = list(items)
    batch[3] = _tampered(pp, items[3], "w_eval", side)
    d = _under_every_mode(pp, batch, [q != 3 for q in range(6)])
    # the entry fails its side's comparison and leaves: a primary failure is not evaluated on the secondary side
    points = 6 + 5 if side == 0 else 6 + 6
    assert d[16] == (2, points, 1) and d[1] == (points, points, 1)
    assert d[2] == (6, points, 1)                                             # 3 + 3 passes: five live entries still take three
    assert batch[3][0].verify(pp, *batch[3][1:]) is False


def test_last_inner_round_element(six):
    pp, items = six
    batch = list(items)
    batch[0] = _tampered(pp, items[0], "inner.last", 0)
    d = _under_every_mode(pp, batch, [False] + [True] * 5)
    assert d[16] == (2, 11, 1)


def test_an_opening_and_a_w_eval_in_two_entries(six):
    """entry 1's sent vector is wrong (only the group check sees it: the combined check fails and every remaining entry is decided
    on its own), entry 4's w_eval is wrong (the deferred comparison sees it first)"""
    pp, items = six
    batch = list(items)
    batch[1] = _tampered(pp, items[1], "ipaW.a0", 0)
    batch[4] = _tampered(pp, items[4], "w_eval", 0)
    d = _under_every_mode(pp, batch, [True, False, True, True, False, True])
    assert d[16] == (2, 11, 1)


def test_wrong_step_count_and_permutation(six):
    pp, items = six
    batch = list(items)
    s, n, z0, zi = items[2]
    batch[2] = (s, n + 1, z0, zi)                                             # an exact check of the replay: never reaches a pass
    d = _under_every_mode(pp, batch, [q != 2 for q in range(6)])
    assert d[16] == (2, 10, 0)
    perm = [4, 2, 5, 0, 3, 1]
    _under_every_mode(pp, [batch[p] for p in perm], [p != 2 for p in perm])
    _under_every_mode(pp, [items[p] for p in perm], [True] * 6)


def test_empty_and_single_batches(six):
    pp, items = six
    _under_every_mode(pp, [], [])
    d = _under_every_mode(pp, [items[5]], [True])
    assert d[16] == (2, 2, 0)


def test_setter_refusals(six):
    pp, _ = six
    pp.set_verify_multi(2)
    for n in (-1, 65):
        with pytest.raises(VdfError) as e:
            pp.set_verify_multi(n)
        assert e.value.code == 1
        assert pp.verify_multi == 2
    pp.set_verify_multi(64)
    assert pp.verify_multi == 64


def test_fp_orientation(ctx):
    pp = public_params(ctx, T, CIRCUIT_MINROOT_REFERENCE, field=FIELD_FP)
    items = []
    for k in range(3):
        initial = State.from_ints(FIELD_FP, o.rand_fe(720 + k, 0, o.P), 0, 1)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(VestaVDF.new_with_mode(FAST), T, STEPS, initial)
        items.append((NovaVDFProof.prove_recursively(pp, circuits, T, z0).compress(pp), STEPS, z0, _zvec(initial)))
    _under_every_mode(pp, items, [True] * 3)
    batch = [items[0], _tampered(pp, items[1], "w_eval", 1, field=FIELD_FP), items[2]]
    d = _under_every_mode(pp, batch, [True, False, True])
    assert d[16] == (2, 6, 1)
    for it in items:
        it[0].free()
    pp.free()


def test_lanes_parameters(ctx):
    L = 2
    pp = public_params_lanes(ctx, T, L)
    vdf = PallasVDF.new_with_mode(FAST)
    items = []
    for k in range(3):
        inits = [State.from_ints(FIELD_FQ, o.rand_fe(740 + k, l, o.Q), 0, 5 * l) for l in range(L)]
        z0, lc = LaneCircuits.begin(T, inits)
        states = list(inits)
        for _ in range(STEPS):
            res = [vdf.eval_with_trace(s, T) for s in states]
            lc.push_traces([r[1] for r in res])
            states = [r[0] for r in res]
        snark = NovaVDFProof.prove_recursively(pp, lc, T, z0).compress(pp)
        items.append((snark, STEPS, z0, [e for s in states for e in _zvec(s)]))
    _under_every_mode(pp, items, [True] * 3)
    batch = [_tampered(pp, items[0], "w_eval", 0), items[1], items[2]]
    d = _under_every_mode(pp, batch, [False, True, True])
    assert d[2] == (2 + 1, 3 + 2, 1)
    for it in items:
        it[0].free()
    pp.free()
