"""GPU: the cross term of a custom circuit's periodic rows without the sparse matrices (include/vdf_hip.h
vdf_nifs_cross_term_periodic, k_nifs_cross_periodic; include/vdf_nova.h tuning.periodic_rows, VDF_STENCIL_PERIODIC).

a. the kernel against the generic sparse kernel over a shape made of the same triples, and against the host evaluator: Az2, Bz2,
   Cz2 and T of the periodic rows byte for byte, guard patterns in front of and behind the range intact; both fields, 3 and 4 rows
   per repetition, row counts on either side of a workgroup of 256;
b. the launcher's refusals, each followed by a valid call;
c. proofs under parameters with periodic_rows = 1 (device and host advice), periodic_rows = 0 and as the plain loop are the same
   bytes, verify and compress to the same bytes; a circuit that is not periodic keeps code 0; inconsistent advice is an
   unsatisfiable witness under code 7 too."""
import numpy as np
import pytest

from oracle import pasta as o
from periodic_spec import GUARD, Acc, described, guarded, operands, refusal_cases
from rounds_spec import F, G, MOD, mont_rows
from util import dev, host, host_trace, ints
from vdf_amd.minroot import PallasVDF, State, VestaVDF
from vdf_amd.nova import (FIELD_FP, FIELD_FQ, STENCIL_PERIODIC, NovaVDFProof, periodic_rows_eval, public_params_custom,
                          shape_digest_custom)

pytestmark = pytest.mark.gpu
LEAD = {"F": 2, "G": 1}


# ---- a. the kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("reps", [2, 3, 64, 65, 86, 257])
@pytest.mark.parametrize("name", ["F", "G"])
def test_a_the_kernel_equals_the_generic_kernel_and_the_host_evaluator(ctx, name, reps, field):
    import torch
    t = reps + LEAD[name]
    mats, pr, info = described(name, t, field)
    assert pr is not None and pr.lead == LEAD[name] and pr.row_count == reps * pr.c.n_cons
    nc, ncols = info["num_cons"], info["num_cols"]
    z2, a1, b1, c1, u1 = operands(field, info, pr, seed=reps + 1000 * field)
    call = (pr.lead, reps, info["seg_begin"], pr.row_begin, ncols, nc)
    want = guarded(nc)
    periodic_rows_eval(field, pr, *call, z2, a1, b1, c1, u1, *want)
    d_in = [dev(x) for x in (z2, a1, b1, c1)]
    got = [dev(g) for g in guarded(nc)]
    ctx.nifs_cross_term_periodic(field, pr, *call, *d_in, u1, *got)
    shape = ctx.shape_create(field, nc, ncols, mats)
    generic = [torch.zeros((nc, 4), dtype=torch.int64, device="cuda") for _ in range(4)]
    ctx.nifs_cross_term(shape, *d_in, u1, *generic)
    ctx.sync()
    lo, hi = pr.row_begin, pr.row_begin + pr.row_count
    for g, w, s in zip(got, want, generic):
        g, s = host(g), host(s)
        assert g[lo:hi].tobytes() == w[lo:hi].tobytes()              # the host evaluator
        assert g[lo:hi].tobytes() == s[lo:hi].tobytes()              # the sparse kernel over the same triples
        assert (g[:lo] == GUARD).all() and (g[hi:] == GUARD).all()
    shape.free()


# ---- b. refusals ------------------------------------------------------------------------------------------------------------------
def test_b_the_launcher_refuses_a_malformed_description_and_then_runs_a_valid_one(ctx):
    from vdf_amd.hip import VdfError
    t, field = 5, FIELD_FQ
    mats, pr, info = described("F", t, field)
    nc = info["num_cons"]
    z2, a1, b1, c1, u1 = operands(field, info, pr, seed=2)
    call = dict(j_first=pr.lead, reps=t - pr.lead, seg_begin=info["seg_begin"], row_begin=pr.row_begin, num_cols=info["num_cols"], num_cons=nc)
    want = guarded(nc)
    periodic_rows_eval(field, pr, *call.values(), z2, a1, b1, c1, u1, *want)
    d_in = [dev(x) for x in (z2, a1, b1, c1)]

    def valid(name):
        got = [dev(g) for g in guarded(nc)]
        ctx.nifs_cross_term_periodic(field, pr, *call.values(), *d_in, u1, *got)
        ctx.sync()
        assert [host(g).tobytes() for g in got] == [w.tobytes() for w in want], name

    def refused(name, args):
        got = [dev(g) for g in guarded(nc)]
        with pytest.raises(VdfError) as e:
            ctx.nifs_cross_term_periodic(field, pr, *args(got))
        assert e.value.code == 1, name                    # VDF_ERR_BAD_ARG
        ctx.sync()
        assert all((host(g) == GUARD).all() for g in got), name

    for name, mutate, over in refusal_cases(pr, info, t):
        undo = mutate()
        refused(name, lambda got: (*{**call, **over}.values(), *d_in, u1, *got))
        undo()
        valid(name)
    # a device pointer where host memory is read, and the reverse
    refused("u1 in device memory", lambda got: (*call.values(), *d_in, dev(u1), *got))
    valid("u1 in device memory")
    refused("z2 in host memory", lambda got: (*call.values(), z2, *d_in[1:], u1, *got))
    valid("z2 in host memory")
    refused("an output in host memory", lambda got: (*call.values(), *d_in, u1, *got[:3], guarded(nc)[0]))
    valid("an output in host memory")
    keep = pr.c.consts
    d_consts = dev(pr.consts)
    pr.c.consts = d_consts.data_ptr()
    refused("the constants in device memory", lambda got: (*call.values(), *d_in, u1, *got))
    pr.c.consts = keep
    valid("the constants in device memory")
    none = [dev(g) for g in guarded(nc)]
    ctx.nifs_cross_term_periodic(field, pr, *{**call, "reps": 0}.values(), *d_in, u1, *none)      # reps = 0 does nothing
    ctx.sync()
    assert all((host(g) == GUARD).all() for g in none)


# ---- c. proofs ----------------------------------------------------------------------------------------------------------------------
VDF = {FIELD_FQ: PallasVDF, FIELD_FP: VestaVDF}


def chain_f(field, t, n):
    """n steps of t MinRoot rounds: z0, zi, per step (advice array, advice ints)"""
    m = MOD[field]
    vdf, s = VDF[field].new(), State.from_ints(field, 0x9E81 + t, 0, 11)
    z0, steps = [s.x, s.y, s.i], []
    for _ in range(n):
        s, tr = host_trace(vdf, s, t)
        steps.append((tr, [o.from_mont(v, m) for v in ints(tr)]))
    return z0, [s.x, s.y, s.i], steps


def chain_g(field, t, n):
    m = MOD[field]
    rng = np.random.default_rng(t)
    k, a = 0x9E3779B97F4A7C15 % m, 0xABCDEF
    fe = lambda v: mont_rows([v], m).tobytes()
    z0, steps = [fe(a), fe(k)], []
    for _ in range(n):
        adv = G.advice_for(a, k, t, m, rng)
        a = adv[3 * t]
        steps.append((mont_rows(adv, m), adv))
    return z0, [fe(a), fe(k)], steps


def prove(ctx, circuit, steps, z0, advice_of, **tune):
    pp = public_params_custom(ctx, circuit, field=circuit.field, **tune)
    proof, keep = None, []
    for arr, as_ints in steps:
        circuit.advice, circuit.advice_ints = advice_of(arr), as_ints
        keep.append(circuit.advice)
        proof = NovaVDFProof.prove_step_custom(pp, proof, circuit, z0)
    ctx.sync()
    return pp, proof


def same_proof_every_way(ctx, cls, chain, field, t, n=3):
    z0, zi, steps = chain(field, t, n)
    runs = [prove(ctx, cls(t, "repeat", field), steps, z0, dev, periodic_rows=1),
            prove(ctx, cls(t, "repeat", field), steps, z0, lambda a: a, periodic_rows=1),
            prove(ctx, cls(t, "repeat", field), steps, z0, dev, periodic_rows=0),
            prove(ctx, cls(t, "loop", field), steps, z0, lambda a: None, periodic_rows=1)]
    assert [pp.stencil() for pp, _ in runs] == [STENCIL_PERIODIC, STENCIL_PERIODIC, 0, 0]
    rows = runs[0][0].periodic_rows()
    assert rows is not None and rows["lead"] == LEAD[cls.__name__]
    assert rows["row_count"] == (t - rows["lead"]) * {"F": 3, "G": 4}[cls.__name__] and rows == runs[2][0].periodic_rows()
    assert runs[3][0].periodic_rows() is None
    assert len({pp.digest() for pp, _ in runs}) == 1                 # the digest does not depend on periodic_rows
    if field == FIELD_FQ:
        assert runs[0][0].digest() == shape_digest_custom(cls(t, "repeat", field))[0]
    blobs = [proof.serialize() for _, proof in runs]
    assert blobs[0] == blobs[3] and blobs[1] == blobs[3] and blobs[2] == blobs[3]
    for pp, proof in runs:
        assert proof.verify(pp, n, z0, zi) is True
        assert proof.verify(pp, n, z0, zi[::-1] if len(zi) == 2 else [zi[1], zi[0], zi[2]]) is False
    snarks = [proof.compress(pp) for pp, proof in runs]
    for (pp, _), s in zip(runs, snarks):
        assert s.verify(pp, n, z0, zi) is True
    wires = [s.serialize() for s in snarks]
    assert wires[0] == wires[3] and wires[1] == wires[3] and wires[2] == wires[3]
    for s in snarks:
        s.free()
    for pp, proof in runs:
        proof.free(); pp.free()


@pytest.mark.parametrize("t", [5, 65])
@pytest.mark.parametrize("name", ["F", "G"])
def test_c_the_same_proof_with_and_without_the_periodic_kernel(ctx, name, t):
    cls, chain = {"F": (F, chain_f), "G": (G, chain_g)}[name]
    same_proof_every_way(ctx, cls, chain, FIELD_FQ, t)


def test_c_the_same_proof_in_the_other_orientation(ctx):
    same_proof_every_way(ctx, F, chain_f, FIELD_FP, 5)


def test_c_a_circuit_that_is_not_periodic_keeps_the_generic_kernel(ctx):
    t, n, field = 5, 3, FIELD_FQ
    m = MOD[field]
    rng = np.random.default_rng(5)
    fe = lambda v: mont_rows([v], m).tobytes()
    a, k = 0x1234, 77
    z0, steps = [fe(a), fe(k)], []
    for _ in range(n):
        adv = Acc.advice_for(a, t, m, rng)
        a = adv[2 * t]
        steps.append((mont_rows(adv, m), adv))
    for advice_of in (dev, lambda x: x):
        pp, proof = prove(ctx, Acc(t, "repeat", field), steps, z0, advice_of, periodic_rows=1)
        assert pp.stencil() == 0 and pp.periodic_rows() is None
        assert proof.verify(pp, n, z0, [fe(a), fe(k)]) is True
        assert proof.verify(pp, n, z0, [fe(a + 1), fe(k)]) is False
        proof.free(); pp.free()


def test_c_inconsistent_advice_is_an_unsatisfiable_witness_under_the_periodic_kernel(ctx):
    t, n, field = 65, 3, FIELD_FQ
    z0, zi, steps = chain_f(field, t, n)
    wrong = [(arr.copy(), as_ints) for arr, as_ints in steps]
    wrong[1][0][t // 2, 0] ^= np.uint64(1)                   # one altered root in the middle of the second step's advice
    for advice_of in (dev, lambda x: x):
        pp, proof = prove(ctx, F(t, "repeat", field), wrong, z0, advice_of, periodic_rows=1)
        assert pp.stencil() == STENCIL_PERIODIC
        assert proof.zi()[0].tobytes() == b"".join(zi)       # the last entries are intact: the statement is the chain's
        assert proof.verify(pp, n, z0, zi) is False
        proof.free(); pp.free()
