"""GPU: compression of many proofs at once (vdf_nova_compress_batch) and the batched passes under it (vdf_reduce_batch,
vdf_fold_halves_batch, vdf_spmv3_t_batch).  The kernels are compared with a big-int restatement of the formulas in
include/vdf_hip.h and with the single calls, bit for bit; every compressed proof of a batch with what proof.compress(pp)
gives for it alone, byte for byte, and one of them with the oracle's compress."""
import time

import numpy as np
import pytest

from oracle import nova as nv, pasta as o, wire as w
from test_gpu_compress import oracle_proof
from test_gpu_seam import Cubic, fe
from test_gpu_snark import BIG_N, ONES, SKEWED_CONS, big_reduction, skewed_eq, skewed_shape, spmvt_formula
from util import ints, mont, unmont, rand_limbs
from vdf_amd.minroot import PallasVDF, State, FIELD_FQ
from vdf_amd.nova import (InverseMinRootCircuit, NovaVDFProof, CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT,
                          compress_batch, public_params, public_params_custom, shape_export, verify_compressed_batch)

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view("<u8")


def _rand(rng, m, k):
    return [int(x) % m for x in ints(rand_limbs(rng, k))]


def _zi(init_ints):
    s = State.from_ints(FIELD_FQ, *init_ints)
    return [s.x, s.y, s.i]


# ---- vdf_reduce_batch ------------------------------------------------------------------------------------------------
def _reduce_formula(kind, tabs, u, n, m):
    if kind == 0:
        return [sum(a * b for a, b in zip(tabs[0], tabs[1])) % m]
    h = n // 2
    at = lambda f, i, t: (f[i] + t * (f[h + i] - f[i])) % m
    if kind == 1:
        return [sum(at(tabs[0], i, t) * at(tabs[1], i, t) for i in range(h)) % m for t in (0, 2)]
    if kind == 2:
        return [sum(at(tabs[0], i, t) * ((at(tabs[1], i, t) * at(tabs[2], i, t) - u * at(tabs[3], i, t) - at(tabs[4], i, t)) % m)
                    for i in range(h)) % m for t in (0, 2, 3)]
    return [sum(tabs[0][i] * tabs[1][h + i] for i in range(h)) % m, sum(tabs[0][h + i] * tabs[1][i] for i in range(h)) % m]


@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("count", [1, 3, 17])
@pytest.mark.parametrize("n", [2, 512, 1 << 13])
def test_reduce_batch_matches_the_formula_and_single_calls(ctx, field, kind, count, n):
    m = o.modulus(field)
    rng = np.random.default_rng(100 * kind + 10 * count + field + n)
    ntab = 5 if kind == 2 else 2
    tabs = [[_rand(rng, m, n) for _ in range(ntab)] for _ in range(count)]
    us = _rand(rng, m, count)
    dev = [[_dev(mont(t, m)) for t in ts] for ts in tabs]
    u = np.stack([mont([x], m)[0] for x in us]) if kind == 2 else None
    got = ctx.reduce_batch(field, kind, dev, n, u=u)
    for q in range(count):
        single = ctx.reduce(field, kind, dev[q], n, u=mont([us[q]], m) if kind == 2 else None)
        assert np.array_equal(got[q], single), q
        assert unmont(got[q], m) == _reduce_formula(kind, tabs[q], us[q], n, m), q


@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_reduce_batch_of_one_above_the_grid_cap(ctx, field, kind):
    """count = 1 at n = 2^19: 512 workgroups for the instance, so the final pass takes two partials per lane."""
    tabs, u, exp = big_reduction(field)
    dev = [_dev(t) for t in tabs[:5 if kind == 2 else 2]]
    got = ctx.reduce_batch(field, kind, [dev], BIG_N, u=u if kind == 2 else None)
    assert ints(got[0]) == (exp["dot", BIG_N, 0, 1] if kind == 0 else exp[kind, BIG_N])
    assert np.array_equal(got[0], ctx.reduce(field, kind, dev, BIG_N, u=u if kind == 2 else None))


@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("count", [2, 3])
def test_dot_product_batch_strides(ctx, field, count):
    """n = 2^18 needs 1024 workgroups per instance: count = 2 gives each 256 of four strides, count = 3 gives each 170 (not a power
    of two: the strides end unevenly)."""
    n = 1 << 18
    tabs, _, exp = big_reduction(field)
    dev = [_dev(t[:n]) for t in tabs[:count + 1]]
    got = ctx.reduce_batch(field, 0, [[dev[q], dev[q + 1]] for q in range(count)], n)
    for q in range(count):
        assert ints(got[q]) == exp["dot", n, q, q + 1], q
        assert np.array_equal(got[q], ctx.reduce(field, 0, [dev[q], dev[q + 1]], n)), q


def test_reduce_batch_refuses_bad_arguments(ctx):
    d = _dev(np.zeros((8, 4), dtype="<u8"))
    with pytest.raises(Exception):
        ctx.reduce_batch(o.FIELD_FQ, 1, [[d, d]], 6)                    # a round needs a power of two
    with pytest.raises(Exception):
        ctx.reduce_batch(o.FIELD_FQ, 0, [[d, d]] * 513, 8)              # more instances than the scratch holds
    assert ctx.reduce_batch(o.FIELD_FQ, 0, [], 8).shape == (0, 1, 4)


# ---- vdf_fold_halves_batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("k,n", [(9, 2), (20, 64), (40, 1 << 10), (13, 1 << 14), (320, 8)])
def test_fold_halves_batch_folds_each_vector_with_its_own_coefficients(ctx, field, k, n):
    m = o.modulus(field)
    rng = np.random.default_rng(7 * k + n + field)
    vs = [_rand(rng, m, n) for _ in range(k)]
    lo, hi = _rand(rng, m, k), _rand(rng, m, k)
    dv = [_dev(mont(v, m)) for v in vs]
    ctx.fold_halves_batch(field, dv, mont(lo, m), mont(hi, m), n)
    ctx.sync()
    h = n // 2
    for t in range(k):
        got = unmont(_host(dv[t]), m)
        assert got[:h] == [(lo[t] * vs[t][i] + hi[t] * vs[t][h + i]) % m for i in range(h)], t
        assert got[h:] == vs[t][h:], t                                  # upper half untouched


def test_fold_halves_batch_refuses_more_than_320_vectors(ctx):
    d = _dev(np.zeros((4, 4), dtype="<u8"))
    c = np.zeros((321, 4), dtype="<u8")
    with pytest.raises(Exception):
        ctx.fold_halves_batch(o.FIELD_FQ, [d] * 321, c, c, 4)


# ---- vdf_spmv3_t_batch -----------------------------------------------------------------------------------------------
def _check_spmv_batch(ctx, shape, field, num_cons, ncols, count, seed):
    m = o.modulus(field)
    rng = np.random.default_rng(seed)
    eqs = [_dev(mont(_rand(rng, m, num_cons), m)) for _ in range(count)]
    rhos = _rand(rng, m, count)
    outs = [_dev(np.full((ncols, 4), 0xFFFFFFFFFFFFFFFF, dtype="<u8")) for _ in range(count)]   # garbage: all written
    ctx.spmv3_t_batch(shape, eqs, np.stack([mont([r], m)[0] for r in rhos]), outs)
    ctx.sync()
    for q in range(count):
        one = _dev(np.zeros((ncols, 4), dtype="<u8"))
        ctx.spmv3_t(shape, eqs[q], mont([rhos[q]], m), one)
        ctx.sync()
        assert np.array_equal(_host(outs[q]), _host(one)), q


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("count", [1, 2, 8])
def test_spmv3_t_batch_on_both_sides_of_t_1024(ctx, side, count):
    mats = shape_export(1024, CIRCUIT_MINROOT_REFERENCE, side)
    field = o.FIELD_FQ if side == 0 else o.FIELD_FP
    num_cons = int(max(int(r.max()) for r, _, _ in mats if r.size)) + 1
    ncols = int(max(int(c.max()) for _, c, _ in mats if c.size)) + 1
    shape = ctx.shape_create(field, num_cons, ncols, mats)
    _check_spmv_batch(ctx, shape, field, num_cons, ncols, count, 31 * side + count)
    shape.free()


@pytest.mark.parametrize("count", [1, 2, 8])
def test_spmv3_t_batch_heavy_columns(ctx, count):
    """Columns of more than SPMVT_HEAVY (64) entries: one of 3000 and several of 100, one workgroup each (a column is shared by
    64 workgroups only past 4096 entries: test_spmv3_t_batch_skewed_columns)."""
    field, m = o.FIELD_FQ, o.Q
    rng = np.random.default_rng(5 + count)
    num_cons, ncols = 4096, 40
    ents = [[], [], []]
    for r in range(3000):
        ents[r % 3].append((r, 0))                                      # the long column
    for c in range(1, 9):
        for r in rng.choice(num_cons, 100, replace=False):
            ents[int(r) % 3].append((int(r), c))
    for c in range(9, ncols):
        for r in rng.choice(num_cons, 5, replace=False):
            ents[int(r) % 3].append((int(r), c))
    mats = []
    for es in ents:
        vals = _rand(rng, m, len(es))
        vals[:3] = [1, m - 1, 2]                                        # the dictionary's +1 and -1, and a plain value
        mats.append((np.array([e[0] for e in es], dtype=np.uint32), np.array([e[1] for e in es], dtype=np.uint32), mont(vals, m)))
    shape = ctx.shape_create(field, num_cons, ncols, mats)
    _check_spmv_batch(ctx, shape, field, num_cons, ncols, count, 77 + count)
    shape.free()


@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("profile", ["few-big", "many-big"])
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 7, 8])
def test_spmv3_t_batch_skewed_columns(ctx, count, profile, field):
    """The batch against the formula over the COO triples (test_gpu_snark.skewed_shape), each instance with its own eq and rho:
    widths 1, 2 and 4, the widest with cnt < 4 (3; 5 = 4 + 1, 7 = 4 + 3), columns shared by 64 workgroups within the scratch's
    room (few-big) and past it (many-big: 12, 24 and 30 columns from heavy + shared).  One instance has rho = 0 and one rho = 1;
    where that leaves no other (count <= 2), a second call has random ones."""
    m = o.modulus(field)
    mats, triples, ncols = skewed_shape(profile, field)
    shape = ctx.shape_create(field, SKEWED_CONS, ncols, mats)
    rng = np.random.default_rng(1000 * count + 10 * ncols + field)
    base = _rand(rng, m, count)
    rho_sets = [[0], [1], base] if count == 1 else [[0] + base[1:-1] + [1]] + ([base] if count == 2 else [])
    for rhos in rho_sets:
        eqs = [skewed_eq(rng, m) for _ in range(count)]
        outs = [_dev(np.full((ncols, 4), ONES, dtype="<u8")) for _ in range(count)]
        ctx.spmv3_t_batch(shape, [_dev(mont(e, m)) for e in eqs], np.stack([mont([r], m)[0] for r in rhos]), outs)
        ctx.sync()
        for q in range(count):
            exp = spmvt_formula(triples, eqs[q], rhos[q], ncols, m)
            assert exp[0] == 0 and ints(_host(outs[q])) == ints(mont(exp, m)), (rhos[q], q)
    shape.free()


# ---- vdf_nova_compress_batch -----------------------------------------------------------------------------------------
def _proofs(pp, ctx, t, specs, kind):
    """[(proof, num_steps, z0, zi, initial state)] of chains with their own seeds and lengths under pp (as test_gpu_nova.make
    builds one, without a parameter set of its own)."""
    out = []
    for seed, n in specs:
        init_ints = (o.rand_fe(seed, 0, o.Q), 0, 1)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, n, State.from_ints(FIELD_FQ, *init_ints))
        out.append((NovaVDFProof.prove_recursively(pp, circuits, t, z0), n, z0, _zi(init_ints), init_ints))
    return out


@pytest.mark.parametrize("t,kind", [(5, CIRCUIT_MINROOT_REFERENCE), (5, CIRCUIT_MINROOT_BOUND), (1024, CIRCUIT_MINROOT_REFERENCE),
                                    (1024, CIRCUIT_MINROOT_BOUND)], ids=["t5-reference", "t5-bound", "t1024-reference", "t1024-bound"])
def test_batch_bytes_equal_single_compress(ctx, t, kind):
    pp = public_params(ctx, t, kind, GENS_TRY_AND_INCREMENT)
    items = _proofs(pp, ctx, t, [(11, 1), (12, 2), (13, 3)], kind)
    got = compress_batch(pp, [it[0] for it in items])
    assert len(got) == 3
    for s, it in zip(got, items):
        assert s.serialize() == it[0].compress(pp).serialize()
    assert verify_compressed_batch(pp, [(s,) + it[1:4] for s, it in zip(got, items)]) == [True] * 3
    if t == 5:                                                          # one of them against the oracle
        _, n, _, _, init_ints = items[2]
        opp, want_s, _ = oracle_proof(t, n, init_ints, bound=(kind == CIRCUIT_MINROOT_BOUND))
        assert got[2].serialize() == w.encode_compressed_proof(t, opp.params, nv.compress(opp, want_s))


def test_batch_of_a_custom_step_circuit(ctx):
    circuit = Cubic()
    pp = public_params_custom(ctx, circuit)
    proofs, finals = [], []
    for x0, n in ((0x1234567, 1), (0x42, 2), (0x777, 3)):
        proof, x = _cubic_chain(pp, circuit, x0, n)
        proofs.append(proof)
        finals.append((n, [fe(x0)], [fe(x)]))
    got = compress_batch(pp, proofs)
    for s, p, (n, z0, zi) in zip(got, proofs, finals):
        assert s.serialize() == p.compress(pp).serialize()
        assert s.verify(pp, n, z0, zi)


def test_queue_settings_change_no_byte(ctx):
    t = 1024
    out = []
    for q in (0, 1):
        pp = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT, compress_queues=q)
        assert pp.tuning()["compress_queues"] == q
        items = _proofs(pp, ctx, t, [(21, 1), (22, 2)], CIRCUIT_MINROOT_REFERENCE)
        got = [s.serialize() for s in compress_batch(pp, [it[0] for it in items])]
        assert got == [it[0].compress(pp).serialize() for it in items]
        out.append(got)
    assert out[0] == out[1]


def _cubic_chain(pp, circuit, x0, n):
    proof, x = None, x0
    for _ in range(n):
        proof = NovaVDFProof.prove_step_custom(pp, proof, circuit, [fe(x0)])
        x = (x ** 3 + x + 5) % o.Q
    return proof, x


def test_a_proof_named_twice(ctx):
    circuit = Cubic()
    pp = public_params_custom(ctx, circuit)
    a, xa = _cubic_chain(pp, circuit, 0x99, 2)
    b, _ = _cubic_chain(pp, circuit, 0x55, 1)
    got = compress_batch(pp, [a, b, a])
    assert got[0].serialize() == got[2].serialize() == a.compress(pp).serialize()
    assert got[1].serialize() == b.compress(pp).serialize()
    want = got[2].serialize()
    got[0].free()                                                       # each copy is freed on its own
    assert got[2].serialize() == want and got[2].verify(pp, 2, [fe(0x99)], [fe(xa)])
    got[2].free()
    # the proof goes on: one more step, and its compression is still what a fresh single compress gives
    assert a.verify(pp, 2, [fe(0x99)], [fe(xa)])
    NovaVDFProof.prove_step_custom(pp, a, circuit, [fe(0x99)])
    xa = (xa ** 3 + xa + 5) % o.Q
    assert a.verify(pp, 3, [fe(0x99)], [fe(xa)])
    [again] = compress_batch(pp, [a, a])[:1]
    assert again.serialize() == a.compress(pp).serialize()
    assert again.verify(pp, 3, [fe(0x99)], [fe(xa)])


def test_eleven_proofs_cross_the_lockstep_width(ctx):
    t = 5
    pp = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    items = _proofs(pp, ctx, t, [(40 + k, 1 + k % 3) for k in range(11)], CIRCUIT_MINROOT_REFERENCE)
    got = compress_batch(pp, [it[0] for it in items])
    for s, it in zip(got, items):
        assert s.serialize() == it[0].compress(pp).serialize()
    assert verify_compressed_batch(pp, [(s,) + it[1:4] for s, it in zip(got, items)]) == [True] * 11


def test_batch_argument_errors(ctx):
    t = 5
    pp = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    assert compress_batch(pp, []) == []
    (a, *_), (b, *_) = _proofs(pp, ctx, t, [(51, 1), (52, 2)], CIRCUIT_MINROOT_REFERENCE)
    pp2 = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    (other, *_), = _proofs(pp2, ctx, t, [(53, 1)], CIRCUIT_MINROOT_REFERENCE)
    with pytest.raises(Exception, match="entry 2"):
        compress_batch(pp, [a, b, other])
    with pytest.raises(Exception, match="entry 1"):
        compress_batch(pp, [a, None, b])
    # nothing was disturbed: the batch still compresses
    assert [s.serialize() for s in compress_batch(pp, [b, a])] == [b.compress(pp).serialize(), a.compress(pp).serialize()]


def test_full_size_two_proofs_t_2_16(ctx):
    t = 1 << 16
    pp = public_params(ctx, t, CIRCUIT_MINROOT_REFERENCE, GENS_TRY_AND_INCREMENT)
    items = _proofs(pp, ctx, t, [(61, 2), (62, 2)], CIRCUIT_MINROOT_REFERENCE)
    proofs = [it[0] for it in items]
    compress_batch(pp, proofs)                                          # warm
    t0 = time.perf_counter()
    got = compress_batch(pp, proofs)
    batch_ms = (time.perf_counter() - t0) * 1e3 / 2
    t0 = time.perf_counter()
    single = [p.compress(pp) for p in proofs]
    single_ms = (time.perf_counter() - t0) * 1e3 / 2
    print(f"t = 2^16, K = 2: batch {batch_ms:.1f} ms per proof, single {single_ms:.1f} ms per proof")
    for s, one in zip(got, single):
        assert s.serialize() == one.serialize()
    assert verify_compressed_batch(pp, [(s,) + it[1:4] for s, it in zip(got, items)]) == [True, True]
