"""GPU: batch verification of running proofs (vdf_nova_verify_batch) and the two kernels under it, the random linear
combination of many vectors (vdf_lincomb_u128) and the combined relaxed R1CS residual of many instances of one shape
(vdf_relaxed_residual_batch).  The kernels are compared with big-int restatements of their formulas; the batch verifier's
verdicts with the single verifier's, entry by entry, under tampering, swapped statements, opposite errors in two copies of
one proof and a witness that breaks a constraint behind consistent commitments."""
import ctypes as C

import numpy as np
import pytest

from oracle import pasta as o
from test_gpu_seam import Cubic, fe
from util import ints, mont, unmont, rand_limbs
from vdf_amd.hip import Context, VdfError
from vdf_amd.minroot import PallasVDF, State, FIELD_FQ
from vdf_amd.nova import (InverseMinRootCircuit, NovaVDFProof, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT,
                          INST_RUNNING_PRIMARY, INST_RUNNING_SECONDARY, INST_FRESH_SECONDARY, nova_lib, public_params,
                          public_params_custom, shape_export, verify_batch)

pytestmark = pytest.mark.gpu
LONG_ROW = 8                                  # VDF_LONG_ROW (vdf_amd/csrc/internal.h)
SCAL = (o.Q, o.P)                             # scalar modulus of side 0 / 1


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t, n):
    return t.cpu().numpy().view("<u8").reshape(-1, 4)[:n]


def _rand(rng, m, k):
    return [int(x) % m for x in ints(rand_limbs(rng, k))]


def _w128(vals):
    return np.array([[v & (2**64 - 1), v >> 64, 0, 0] for v in vals], dtype="<u8").reshape(-1, 4)


# ---- vdf_lincomb_u128 ----------------------------------------------------------------------------------------------------
# (lengths, n_out): one, two, seven and 64 vectors; unequal lengths (zero padding); n_out not a multiple of the 256-lane block
LINCOMB_CASES = [([1000], 1000), ([300, 300], 300), ([5000, 17, 4999, 0, 256, 1, 3000], 5001),
                 ([777 - 9 * j for j in range(64)], 777), ([12345, 200, 12000], 12346)]


@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("case", range(len(LINCOMB_CASES)))
def test_lincomb_u128_matches_the_formula(ctx, field, case):
    lengths, n_out = LINCOMB_CASES[case]
    m = o.modulus(field)
    rng = np.random.default_rng(17 * case + field)
    vecs = [_rand(rng, m, n) if n else [] for n in lengths]
    special = [0, 1, 2**128 - 1]
    ws = [special[j] if j < 3 else int.from_bytes(rng.bytes(16), "little") for j in range(len(lengths))]
    dvecs = [_dev(mont(v, m)) if v else _dev(np.zeros((1, 4), dtype="<u8")) for v in vecs]
    out = _dev(np.full((n_out, 4), 0xFFFFFFFFFFFFFFFF, dtype="<u8"))    # garbage: every entry must be written
    ctx.lincomb_u128(field, dvecs, lengths, _w128(ws), n_out, out)
    ctx.sync()
    got = unmont(_host(out, n_out), m)
    want = [0] * n_out
    for v, w in zip(vecs, ws):
        for i, x in enumerate(v):
            want[i] = (want[i] + w * x) % m
    bad = [i for i in range(n_out) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])


def test_lincomb_u128_refuses_a_weight_of_2_128(ctx):
    m = o.Q
    v = _dev(mont([1, 2, 3], m))
    out = _dev(np.zeros((3, 4), dtype="<u8"))
    w = np.array([[0, 0, 1, 0]], dtype="<u8")
    with pytest.raises(VdfError) as e:
        ctx.lincomb_u128(o.FIELD_FQ, [v], [3], w, 3, out)
    assert e.value.code == 1


# ---- vdf_relaxed_residual_batch ------------------------------------------------------------------------------------------
def _shape(ctx, side, t=1024):
    mats = shape_export(t, CIRCUIT_MINROOT_REFERENCE, side)
    field = o.FIELD_FQ if side == 0 else o.FIELD_FP
    num_cons = int(max(int(r.max()) for r, _, _ in mats if r.size)) + 1
    ncols = int(max(int(c.max()) for _, c, _ in mats if c.size)) + 1
    return mats, field, num_cons, ncols, ctx.shape_create(field, num_cons, ncols, mats)


def _products(mats, m, num_cons, z):
    out = []
    for rows, cols, vals in mats:
        acc = [0] * num_cons
        for r, c, v in zip(rows.tolist(), cols.tolist(), unmont(vals, m)):
            acc[r] = (acc[r] + v * z[c]) % m
        out.append(acc)
    return out


@pytest.mark.parametrize("side", [0, 1])
def test_residual_batch_matches_the_formula_at_t_1024(ctx, side):
    mats, field, num_cons, ncols, shape = _shape(ctx, side)
    m = SCAL[side]
    lens = [np.bincount(r, minlength=num_cons) for r, _, _ in mats]
    assert max(int(x.max()) for x in lens) > LONG_ROW                  # rows that take a wavefront each are in the pass
    rng = np.random.default_rng(91 + side)
    count = 3
    zs = [_rand(rng, m, ncols) for _ in range(count)]
    Es = [_rand(rng, m, num_cons), None, _rand(rng, m, num_cons)]       # a NULL E is the zero vector
    us = _rand(rng, m, count)
    rhos = [int.from_bytes(rng.bytes(16), "little") for _ in range(count)]
    out = _dev(np.full((num_cons, 4), 0xFFFFFFFFFFFFFFFF, dtype="<u8"))
    ctx.relaxed_residual_batch(shape, [_dev(mont(z, m)) for z in zs], [None if e is None else _dev(mont(e, m)) for e in Es],
                               mont(us, m), _w128(rhos), out)
    ctx.sync()
    got = unmont(_host(out, num_cons), m)
    want = [0] * num_cons
    for z, E, u, rho in zip(zs, Es, us, rhos):
        a, b, c = _products(mats, m, num_cons, z)
        for r in range(num_cons):
            want[r] = (want[r] + rho * (a[r] * b[r] - u * c[r] - (E[r] if E else 0))) % m
    bad = [r for r in range(num_cons) if got[r] != want[r]]
    assert not bad, (len(bad), bad[:8])
    shape.free()


def test_residual_of_real_witnesses_is_zero(ctx):
    t = 1024
    pp = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    proof = _chains(pp, t, [(3, 2)])[0][0]
    for side in (0, 1):
        mats, field, num_cons, ncols, shape = _shape(ctx, side, t)
        m = SCAL[side]
        whiches = (INST_RUNNING_PRIMARY,) if side == 0 else (INST_RUNNING_SECONDARY, INST_FRESH_SECONDARY)
        zs, Es, us = [], [], []
        for which in whiches:
            z, E = proof.witness(which)
            zs.append(_dev(z))
            Es.append(None if E is None else _dev(E))
            us.append(np.ascontiguousarray(proof.instance(which)["u"]).reshape(4))
        rho = _w128([2**128 - 1 - k for k in range(len(whiches))])
        out = _dev(np.full((num_cons, 4), 0xFFFFFFFFFFFFFFFF, dtype="<u8"))
        ctx.relaxed_residual_batch(shape, zs, Es, np.stack(us), rho, out)
        ctx.sync()
        assert not _host(out, num_cons).any()
        shape.free()


# ---- vdf_nova_verify_batch -----------------------------------------------------------------------------------------------
def _zi(init_ints):
    s = State.from_ints(FIELD_FQ, *init_ints)
    return [s.x, s.y, s.i]


def _chains(pp, t, specs):
    """[(proof, num_steps, z0, zi)] of MinRoot chains with their own seeds and lengths under pp."""
    out = []
    for seed, n in specs:
        init_ints = (o.rand_fe(seed, 0, o.Q), 0, 1)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, n, State.from_ints(FIELD_FQ, *init_ints))
        out.append((NovaVDFProof.prove_recursively(pp, circuits, t, z0), n, z0, _zi(init_ints)))
    return out


def _zi_now(proof):
    """the proof's carried zi_primary, element by element (Montgomery bytes)"""
    zp = np.ascontiguousarray(proof.zi()[0]).reshape(-1, 4)
    return [zp[j].tobytes() for j in range(zp.shape[0])]


def _single(pp, items):
    return [it[0].verify(pp, it[1], it[2], it[3]) for it in items]


@pytest.fixture(scope="module")
def batch_1024():
    ctx = Context(0)
    t = 1024
    pp = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    items = _chains(pp, t, [(21, 1), (22, 2), (23, 3), (24, 1), (25, 2), (26, 3)])
    yield ctx, pp, items


def _word(ctx, addr, value=None):
    from vdf_amd._lib import lib
    w = np.zeros(1, dtype="<u8")
    if value is None:
        ctx._check(lib.vdf_dev_memcpy(ctx.handle, w.ctypes.data, addr, 8))
        return int(w[0])
    w[0] = value
    ctx._check(lib.vdf_dev_memcpy(ctx.handle, addr, w.ctypes.data, 8))


def _ptrs(proof, which):
    dz, dE = C.c_void_p(), C.c_void_p()
    assert nova_lib.vdf_nova_proof_witness_ptrs(proof.handle, which, C.byref(dz), C.byref(dE)) == 0
    return dz.value, dE.value


def test_valid_and_permuted_batches(batch_1024):
    ctx, pp, items = batch_1024
    assert _single(pp, items) == [True] * 6
    assert verify_batch(pp, items) == [True] * 6
    perm = [4, 0, 5, 2, 1, 3]
    assert verify_batch(pp, [items[k] for k in perm]) == [True] * 6


def test_one_word_tampering_rejects_that_entry_alone(batch_1024):
    ctx, pp, items = batch_1024
    victim = items[2][0]
    for which in (INST_RUNNING_PRIMARY, INST_RUNNING_SECONDARY, INST_FRESH_SECONDARY):
        dz, dE = _ptrs(victim, which)
        for base, off in ((dz, 32 * 40), (dE, 32 * 11)):
            if not base:
                continue
            word = _word(ctx, base + off)
            _word(ctx, base + off, word ^ 1)
            want = [k != 2 for k in range(6)]
            assert verify_batch(pp, items) == want
            assert _single(pp, items) == want
            _word(ctx, base + off, word)
            assert verify_batch(pp, items) == [True] * 6


def test_wrong_statements_and_a_proof_named_twice(batch_1024):
    ctx, pp, items = batch_1024
    p0, n0, z00, zi0 = items[0]
    p1, n1, z01, zi1 = items[1]
    cases = [(p0, n0 + 1, z00, zi0), (p1, n1, z00, zi1), (p1, n1, zi1, z01), (p0, n0, z00, zi1)]
    mixed = [items[3]] + cases + [items[4], items[4], items[3]]
    want = _single(pp, mixed)
    assert want == [True, False, False, False, False, True, True, True]
    assert verify_batch(pp, mixed) == want


def test_opposite_errors_do_not_cancel(batch_1024):
    ctx, pp, items = batch_1024
    blob = items[1][0].serialize()
    a, b = NovaVDFProof.deserialize(pp, blob), NovaVDFProof.deserialize(pp, blob)
    m, off, delta = o.Q, 32 * 123, 0xDEADBEEF
    for p, sign in ((a, 1), (b, -1)):
        dz, _ = _ptrs(p, INST_RUNNING_PRIMARY)
        limbs4 = [_word(ctx, dz + off + 8 * k) for k in range(4)]
        v = (sum(x << (64 * k) for k, x in enumerate(limbs4)) + sign * delta) % m
        for k in range(4):
            _word(ctx, dz + off + 8 * k, (v >> (64 * k)) & (2**64 - 1))
    n, z0, zi = items[1][1:]
    pair = [(a, n, z0, zi), (b, n, z0, zi)]
    assert verify_batch(pp, pair) == [False, False]
    assert verify_batch(pp, [items[0], pair[0], items[2], pair[1]]) == [True, False, True, False]


class Skewed(Cubic):
    """Cubic with a witness one off in its last variable: the constraint rhs * 1 = y breaks, every commitment and hash is
    made honestly over the wrong witness."""

    def synthesize(self, cs, z):
        x = z[0]
        x2 = cs.mul(x, x)
        x3 = cs.mul(x2, x)
        rhs = cs.add(cs.add(x3, x), cs.const(fe(5)))
        val = None
        if cs.is_witness:
            r = int.from_bytes(cs.value(rhs), "little")
            val = ((r + o.to_mont(1, o.Q)) % o.Q).to_bytes(32, "little")
        y = cs.alloc(val)
        cs.enforce(rhs, cs.const(fe(1)), y)
        return [y]


def test_the_residual_check_catches_what_the_openings_cannot(ctx):
    circuit = Cubic()
    pp = public_params_custom(ctx, circuit)
    good, x = None, 0x1234
    for _ in range(2):
        good = NovaVDFProof.prove_step_custom(pp, good, circuit, [fe(0x1234)])
        x = (x ** 3 + x + 5) % o.Q
    bad = NovaVDFProof.prove_step_custom(pp, None, Skewed(), [fe(0x77)])
    bad_zi = _zi_now(bad)[0]
    items = [(good, 2, [fe(0x1234)], [fe(x)]), (bad, 1, [fe(0x77)], [bad_zi])]
    assert _single(pp, items) == [True, False]
    assert verify_batch(pp, items) == [True, False]
    assert verify_batch(pp, [items[1]]) == [False]


def test_errors_name_the_entry(batch_1024):
    ctx, pp, items = batch_1024
    other = public_params(ctx, 5, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    foreign = _chains(other, 5, [(31, 1)])[0]
    with pytest.raises(VdfError) as e:
        verify_batch(pp, [items[0], items[1], foreign])
    assert e.value.code == 1 and "entry 2" in str(e.value)
    with pytest.raises(VdfError) as e:
        verify_batch(pp, [items[0], (None,) + items[1][1:]])
    assert e.value.code == 1 and "entry 1" in str(e.value)
    assert verify_batch(pp, []) == []
    ok, all_ok = (C.c_int * 1)(), C.c_int(0)
    z = (C.c_uint8 * 32)()
    assert nova_lib.vdf_nova_verify_batch(pp.handle, 0, None, None, z, z, ok, C.byref(all_ok)) == 0 and all_ok.value == 1


def test_checkpoints_in_a_second_context(batch_1024):
    ctx, pp, items = batch_1024
    ctx2 = Context(0)
    pp2 = public_params(ctx2, 1024, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    moved = [(NovaVDFProof.deserialize(pp2, it[0].serialize()),) + it[1:] for it in items[:4]]
    assert verify_batch(pp2, moved) == [True] * 4


@pytest.mark.parametrize("tuning", [{}, {"fold_on_rows": 0}], ids=["default", "fold_on_rows=0"])
def test_verification_changes_nothing_later(ctx, tuning):
    t = 1024
    pp = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT, **tuning)
    init_ints = (o.rand_fe(41, 0, o.Q), 0, 1)
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, 4, State.from_ints(FIELD_FQ, *init_ints))
    plain = None
    for k in range(4):
        plain = NovaVDFProof.prove_step(pp, plain, circuits, k, z0)
    checked = None
    for k in range(2):
        checked = NovaVDFProof.prove_step(pp, checked, circuits, k, z0)
    assert verify_batch(pp, [(checked, 2, z0, _zi_now(checked))]) == [True]
    for k in range(2, 4):
        checked = NovaVDFProof.prove_step(pp, checked, circuits, k, z0)
    assert checked.serialize() == plain.serialize()
    assert verify_batch(pp, [(checked, 4, z0, _zi(init_ints)), (plain, 4, z0, _zi(init_ints))]) == [True, True]


def test_full_size_t_2_16(ctx):
    t = 1 << 16
    pp = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    items = _chains(pp, t, [(51, 1), (52, 2), (53, 1)])
    assert verify_batch(pp, items) == [True] * 3
    dz, _ = _ptrs(items[1][0], INST_RUNNING_PRIMARY)
    word = _word(ctx, dz + 32 * 1000)
    _word(ctx, dz + 32 * 1000, word ^ 1)
    assert verify_batch(pp, items) == [True, False, True]
    _word(ctx, dz + 32 * 1000, word)
    assert verify_batch(pp, items) == [True] * 3
