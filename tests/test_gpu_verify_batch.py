"""GPU: batch verification of compressed proofs (vdf_nova_verify_compressed_batch) and the kernel under it, the inner-product
argument's generator coefficients for many weighted openings (vdf_ipa_coefficients).  The kernel is compared with a big-int
restatement of its formula; the batch verifier's verdicts with the single verifier's, entry by entry, including tampered
proofs, swapped statements and two proofs whose errors cancel under equal weights."""
import numpy as np
import pytest

from oracle import pasta as o
from test_gpu_nova import make
from util import ints, mont, unmont, rand_limbs
from vdf_amd.minroot import PallasVDF, State, FIELD_FQ
from vdf_amd.nova import (CompressedNovaVDFProof, InverseMinRootCircuit, NovaVDFProof, CIRCUIT_MINROOT_REFERENCE,
                          verify_compressed_batch)

pytestmark = pytest.mark.gpu
SCAL = (o.Q, o.P)                      # scalar modulus of side 0 / 1 arguments


# ---- vdf_ipa_coefficients -----------------------------------------------------------------------------------------
def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _rand(rng, m, k):
    return [int(x) % m for x in ints(rand_limbs(rng, k))] if k else []


def _formula(openings, n, m):
    """out[i] = sum_q w_q pattern_q[i mod 2^log_m] prod_j (bit (k-1-j) of (i >> log_m) ? hi[j] : lo[j])"""
    out = [0] * n
    for w, lo, hi, pat in openings:
        k, log_m = len(lo), (len(pat) - 1).bit_length()
        for i in range(min(n, 1 << (k + log_m))):
            e = w * pat[i & ((1 << log_m) - 1)]
            top = i >> log_m
            for j in range(k):
                e = e * (hi[j] if (top >> (k - 1 - j)) & 1 else lo[j]) % m
            out[i] = (out[i] + e) % m
    return out


def _run(ctx, field, openings, n):
    m = o.modulus(field)
    out = _dev(np.full((max(n, 1), 4), 0xFFFFFFFFFFFFFFFF, dtype="<u8"))    # garbage: every entry must be written
    ctx.ipa_coefficients(field, [(mont([w], m), mont(lo, m), mont(hi, m), mont(pat, m)) for w, lo, hi, pat in openings], n, out)
    ctx.sync()
    return out.cpu().numpy().view("<u8")[:n]


# (k, log_m) per opening and the output length: short openings (entry by entry in the kernel), long ones (the product tree),
# an empty pattern-only opening, n past the longest opening and n cutting one short
CASES = [
    ([(0, 0)], 600),
    ([(3, 2)], 100),
    ([(9, 4)], 1 << 13),
    ([(5, 4), (9, 0)], 1 << 10),
    ([(10, 3), (2, 1), (0, 4)], 9000),
    ([(8, 1), (8, 1), (6, 2), (11, 0)], 3000),
    ([(12, 0), (4, 4), (9, 2), (7, 3), (1, 0)], 1 << 12),
    ([(6, 4), (10, 4), (3, 0), (12, 1), (5, 2), (0, 1)], 5000),
    ([(13, 2)], 1 << 14),
    ([(11, 4), (10, 2)], 20000),
]


@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_ipa_coefficients_match_the_formula(ctx, field, case):
    shapes, n = CASES[case]
    m = o.modulus(field)
    rng = np.random.default_rng(1000 * case + field)
    openings = [(_rand(rng, m, 1)[0], _rand(rng, m, k), _rand(rng, m, k), _rand(rng, m, 1 << log_m)) for k, log_m in shapes]
    got = unmont(_run(ctx, field, openings, n), m)
    want = _formula(openings, n, m)
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("field", [o.FIELD_FP, o.FIELD_FQ])
@pytest.mark.parametrize("k,log_m", [(0, 0), (0, 4), (3, 2), (8, 0), (9, 4), (14, 4), (17, 2)])
def test_one_opening_of_weight_one_is_the_pair_table_pattern(ctx, field, k, log_m):
    m = o.modulus(field)
    rng = np.random.default_rng(7 * k + log_m)
    lo, hi, pat = _rand(rng, m, max(k, 1))[:k], _rand(rng, m, max(k, 1))[:k], _rand(rng, m, 1 << log_m)
    n = 1 << (k + log_m)
    want = _dev(np.zeros((n, 4), dtype="<u8"))
    ctx.pair_table_pattern(field, mont(lo, m) if k else None, mont(hi, m) if k else None, k, mont(pat, m), log_m, want)
    got = _run(ctx, field, [(1, lo, hi, pat)], n)
    assert np.array_equal(got, want.cpu().numpy().view("<u8"))


def test_ipa_coefficients_refuse_oversize_openings(ctx):
    m = o.modulus(o.FIELD_FQ)
    out = _dev(np.zeros((64, 4), dtype="<u8"))
    with pytest.raises(Exception):
        ctx.ipa_coefficients(o.FIELD_FQ, [(mont([1], m), mont([1] * 3, m), mont([1] * 3, m), mont([1] * 32, m))], 64, out)   # pattern of 32
    with pytest.raises(Exception):
        ctx.ipa_coefficients(o.FIELD_FQ, [(mont([1], m), mont([1] * 22, m), mont([1] * 22, m), mont([1] * 8, m))], 64, out)  # 25 variables


# ---- vdf_nova_verify_compressed_batch ---------------------------------------------------------------------------------
def _zi(init_ints):
    s = State.from_ints(FIELD_FQ, *init_ints)
    return [s.x, s.y, s.i]


def _chain(pp, t, n, seed):
    """A compressed proof of its own chain under `pp`: (snark, num_steps, z0, zi)."""
    x = o.rand_fe(seed, 0, o.Q)
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, n, State.from_ints(FIELD_FQ, x, 0, 1))
    snark = NovaVDFProof.prove_recursively(pp, circuits, t, z0).compress(pp)
    return snark, n, z0, _zi((x, 0, 1))


def _copy(pp, snark):
    return CompressedNovaVDFProof.deserialize(pp, snark.serialize())


def _single(pp, items):
    return [s.verify(pp, n, z0, zi) for s, n, z0, zi in items]


def _sections(pp, side):
    """Byte offsets of the flat encoding (vdf_nova_snark_bytes) of side `side`'s argument."""
    base = 0
    for sd in range(side + 1):
        sz = pp.sizes(sd)
        s = (sz["num_cons"] - 1).bit_length()
        l1 = (sz["num_vars"] - 1).bit_length() + 1
        kW, kE = (l1 - 1) - 4, s - 4
        head = base + 32 * (3 * s + 4 + 2 * l1 + 1)
        sect = {"claims": base + 32 * 3 * s, "w_eval": base + 32 * (3 * s + 4 + 2 * l1), "ipaW.L0": head, "ipaW.R0": head + 64,
                "ipaW.a0": head + 128 * kW, "ipaE.a15": head + 128 * (kW + kE) + 32 * 31}
        base += 32 * (3 * s + 4 + 2 * l1 + 1 + 16 + 16) + 128 * (kW + kE)
    return sect


def _add_fe(data, off, delta, m):
    v = (int.from_bytes(data[off:off + 32], "little") + delta) % m
    out = bytearray(data)
    out[off:off + 32] = v.to_bytes(32, "little")
    return bytes(out)


T = 1024


@pytest.fixture(scope="module")
def six(ctx):
    pp, z0, circuits, _, init_ints = make(ctx, T, 2, seed=301)
    first = (NovaVDFProof.prove_recursively(pp, circuits, T, z0).compress(pp), 2, z0, _zi(init_ints))
    items = [first] + [_chain(pp, T, 1 + k % 3, 302 + k) for k in range(5)]
    return pp, items


def test_valid_proofs_are_accepted(six):
    pp, items = six
    assert sorted({n for _, n, _, _ in items}) == [1, 2, 3]
    assert verify_compressed_batch(pp, items) == [True] * 6
    for it in items:
        assert verify_compressed_batch(pp, [it]) == [it[0].verify(pp, *it[1:])] == [True]
    assert verify_compressed_batch(pp, [items[2], items[0], items[2], items[2]]) == [True] * 4       # a proof repeated
    assert verify_compressed_batch(pp, []) == []


def test_permuting_a_batch_permutes_the_verdicts(six):
    pp, items = six
    bad = _copy(pp, items[1][0])
    bad.set_bytes(_add_fe(bad.to_bytes(), _sections(pp, 0)["ipaW.a0"], 1, SCAL[0]))
    batch = [items[0], (bad,) + items[1][1:], items[2], items[3]]
    got = verify_compressed_batch(pp, batch)
    assert got == [True, False, True, True]
    perm = [3, 1, 0, 2]
    assert verify_compressed_batch(pp, [batch[p] for p in perm]) == [got[p] for p in perm]


@pytest.mark.parametrize("place,side", [("ipaW.a0", 0), ("ipaE.a15", 1), ("ipaE.a15", 0), ("ipaW.L0", 0), ("ipaW.L0", 1),
                                        ("w_eval", 0), ("claims", 1)])
def test_one_tampered_proof_is_rejected_alone(six, place, side):
    pp, items = six
    sect = _sections(pp, side)
    victim = ["ipaW.a0", "ipaE.a15", "ipaW.L0", "w_eval", "claims"].index(place) % 6
    bad = _copy(pp, items[victim][0])
    data = bad.to_bytes()
    if place == "ipaW.L0":                     # L_0 replaced by another point on the curve (R_0)
        r0 = sect["ipaW.R0"]
        data = data[:sect[place]] + data[r0:r0 + 64] + data[sect[place] + 64:]
    else:
        data = _add_fe(data, sect[place], 1, SCAL[side])
    bad.set_bytes(data)
    batch = list(items)
    batch[victim] = (bad,) + items[victim][1:]
    got = verify_compressed_batch(pp, batch)
    assert got == [q != victim for q in range(6)]
    assert got == _single(pp, batch)


def test_swapped_statements_and_wrong_step_counts_are_rejected(six):
    pp, items = six
    s0, n0, z00, zi0 = items[0]
    s1, n1, z01, zi1 = items[2]
    assert n0 == n1 == 2
    batch = list(items)
    batch[0] = (s0, n0, z01, zi1)              # statements swapped between entries 0 and 2
    batch[2] = (s1, n1, z00, zi0)
    s4, n4, z04, zi4 = items[4]
    batch[4] = (s4, n4 + 1, z04, zi4)          # one step too many
    got = verify_compressed_batch(pp, batch)
    assert got == [False, True, False, True, False, True]
    assert got == _single(pp, batch)


def test_opposite_errors_in_two_proofs_do_not_cancel(six):
    """a is not absorbed before the argument's challenges, so a[0] + d in one copy of a proof and a[0] - d in another give
    exactly opposite errors in the group equation: equal weights would accept the pair."""
    pp, items = six
    off, m = _sections(pp, 0)["ipaW.a0"], SCAL[0]
    good = items[5][0].to_bytes()
    plus, minus = _copy(pp, items[5][0]), _copy(pp, items[5][0])
    plus.set_bytes(_add_fe(good, off, 12345, m))
    minus.set_bytes(_add_fe(good, off, -12345, m))
    rest = items[5][1:]
    assert verify_compressed_batch(pp, [(plus,) + rest, (minus,) + rest]) == [False, False]
    assert verify_compressed_batch(pp, [items[0], (plus,) + rest, items[1], (minus,) + rest]) == [True, False, True, False]


def test_a_proof_under_other_parameters_is_refused(ctx, six):
    import vdf_amd
    pp, items = six
    pp5, z0, circuits, _, init_ints = make(ctx, 5, 2, seed=9)
    other = NovaVDFProof.prove_recursively(pp5, circuits, 5, z0).compress(pp5)
    with pytest.raises(vdf_amd.VdfError) as e:
        verify_compressed_batch(pp, [items[0], items[1], (other, 2, z0, _zi(init_ints))])
    assert e.value.code == 1 and "entry 2" in str(e.value)


def test_proofs_from_bytes_in_a_second_context(six):
    import vdf_amd
    from vdf_amd.nova import public_params
    pp, items = six
    ctx_v = vdf_amd.Context(0)
    pp_v = public_params(ctx_v, T, CIRCUIT_MINROOT_REFERENCE)
    assert pp_v.digest() == pp.digest()
    got = [(CompressedNovaVDFProof.deserialize(pp_v, s.serialize()), n, z0, zi) for s, n, z0, zi in items]
    assert verify_compressed_batch(pp_v, got) == [True] * 6
    for g in got:
        g[0].free()
    pp_v.free()
    ctx_v.close()


def test_three_full_size_proofs_t_2_16(ctx):
    """t = 2^16 (2^19 generators on the primary side): three proofs accepted; one tampered a element rejects that proof only."""
    t = 1 << 16
    pp, z0, circuits, _, init_ints = make(ctx, t, 2, seed=61)
    items = [(NovaVDFProof.prove_recursively(pp, circuits, t, z0).compress(pp), 2, z0, _zi(init_ints))]
    items += [_chain(pp, t, n, seed) for n, seed in ((1, 62), (2, 63))]
    assert verify_compressed_batch(pp, items) == [True] * 3
    bad = _copy(pp, items[1][0])
    bad.set_bytes(_add_fe(bad.to_bytes(), _sections(pp, 0)["ipaW.a0"], 1, SCAL[0]))
    assert verify_compressed_batch(pp, [items[0], (bad,) + items[1][1:], items[2]]) == [True, False, True]
