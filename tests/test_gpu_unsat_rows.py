"""GPU: which row of an instance is unsatisfied (include/vdf_hip.h vdf_unsat_rows, kernel k_unsat_rows; include/vdf_nova.h
vdf_nova_proof_last_unsat, vdf_nova_pp_repeat_rows, VDF_CUSTOM_CHECK_STEPS).

a. the scan against big integers: a partial wavefront, a full one, one lane of a second, a second workgroup, four workgroups;
   no broken row, the first, the last, two of one wavefront, rows of two workgroups, every row; both fields;
b. a round body that disagrees with its chain is named by step, row, repetition and constraint when the steps are checked, and
   stays VDF_OK with a proof that does not verify when they are not;
c. vdf_nova_proof_last_unsat after good steps of a custom circuit and of a built-in kind, and after one wrong advice entry."""
import numpy as np
import pytest

from custom_chain_spec import ENFORCE_INDEX, FC, FW, I0, X0, checkpoints_of, minroot_chain, step_traces, z0_of, zi_of
from oracle import pasta as o
from rounds_spec import MOD, mont_rows
from util import dev
from walks_spec import minroot_body
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError
from vdf_amd.minroot import PallasVDF, State
from vdf_amd.nova import (CustomChain, InverseMinRootCircuit, NovaVDFProof, public_params, public_params_custom, record_walk_body,
                          FIELD_FP, FIELD_FQ)

pytestmark = pytest.mark.gpu
NONE = 2**64 - 1


def patterns(n):
    """the rows to break, by name; a pattern that needs more rows than n is left out for that n"""
    out = {"none": [], "row 0": [0], "row n - 1": [n - 1], "every row": list(range(n))}
    if n >= 2:
        w = (n - 1) // 64 * 64                         # the last wavefront: its first row and the last row of all
        out["two rows of one wavefront"] = [w, n - 1] if w != n - 1 else [w - 2, w - 1]
    if n > 256:
        out["rows of two workgroups"] = [70, 256 + (n - 257) // 2]
    return out


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_the_scan_is_exact(ctx, n, field):
    m = MOD[field]
    rng = np.random.default_rng(n + field)
    a = [int(rng.integers(0, 2**62)) ** 5 % m for _ in range(n)]
    b = [int(rng.integers(0, 2**62)) ** 5 % m for _ in range(n)]
    for k, v in enumerate((0, 1, m - 1)):              # 0, 1 and p - 1 among the operands
        a[(5 * k) % n] = v
        b[(5 * k + 2) % n] = v
    c = [x * y % m for x, y in zip(a, b)]
    d_a, d_b = dev(mont_rows(a, m)), dev(mont_rows(b, m))
    pats = patterns(n)
    assert set(pats) >= {"none", "row 0", "row n - 1", "every row"} and (n < 2 or "two rows of one wavefront" in pats) and \
        (n <= 256 or "rows of two workgroups" in pats)
    for name, rows in pats.items():
        broken = list(c)
        for r in set(rows):
            broken[r] = (broken[r] + 1) % m
        got = ctx.unsat_rows(field, d_a, d_b, dev(mont_rows(broken, m)), n)
        assert got == (len(set(rows)), min(rows) if rows else NONE), (name, rows)


def test_nothing_to_scan_and_a_host_pointer(ctx):
    m = o.Q
    d = dev(mont_rows([1, 2, 3], m))
    assert ctx.unsat_rows(FIELD_FQ, d, d, d, 0) == (0, NONE)
    assert ctx.unsat_rows(FIELD_FQ, None, None, None, 0) == (0, NONE)
    with pytest.raises(VdfError) as e:
        ctx.unsat_rows(FIELD_FQ, mont_rows([1, 2, 3], m), d, d, 3)
    assert e.value.code == VDF_ERR_BAD_ARG
    with pytest.raises(VdfError):
        ctx.unsat_rows(7, d, d, d, 3)
    assert ctx.unsat_rows(FIELD_FQ, d, d, d, 3) == (2, 1)          # 1 * 1 = 1; 2 * 2 != 2; 3 * 3 != 3: the context goes on


def chain_of(field, t, steps, every):
    m = MOD[field]
    tape = record_walk_body(minroot_body(field), field)
    return CustomChain.from_checkpoints(field, tape, mont_rows([I0], m), t, every, steps, checkpoints_of(minroot_chain(field, t, steps), 2, every, m))


def test_a_round_body_that_disagrees_with_the_chain(ctx):
    field, t, steps = FIELD_FQ, 5, 2
    pp = public_params_custom(ctx, FW(t, field), field=field)
    rb, n_cons, reps = pp.repeat_rows()
    assert (n_cons, reps) == (3, t)
    chain = chain_of(field, t, steps, 5)
    assert chain.materialize(ctx, 0, steps) == [0, 0]              # every walk lands on its checkpoint: the chain is a true one
    chain.release()
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, FW(t, field), chain, z0_of(field), window_steps=2, check_steps=True)
    first = rb + 0 * n_cons + ENFORCE_INDEX
    assert e.value.code == VDF_ERR_BAD_ARG
    assert "step 0: %d unsatisfied rows, first row %d (repetition 0, constraint %d of the repeat)" % (t, first, ENFORCE_INDEX) in str(e.value)
    assert chain.memory() == (0, 0)
    # without the flag: the existing rule, pinned
    proof = NovaVDFProof.prove_recursively_custom(pp, FW(t, field), chain, z0_of(field), window_steps=2)
    assert proof.verify(pp, steps, z0_of(field), zi_of(field, t, steps)) is False
    count, row = proof.last_unsat()
    assert (count, row) == (t, first)
    proof.free(); chain.free(); pp.free()


def test_periodic_rows_do_not_matter_to_the_repeat_rows(ctx):
    t = 5
    a = public_params_custom(ctx, FC(t), periodic_rows=0)
    b = public_params_custom(ctx, FC(t), periodic_rows=1)
    assert a.repeat_rows() == b.repeat_rows() and a.repeat_rows()[1:] == (3, t)
    a.free(); b.free()
    pp = public_params(ctx, t)
    assert pp.repeat_rows() is None
    pp.free()


def test_last_unsat_after_good_steps_and_after_one_wrong_entry(ctx):
    field, t, steps = FIELD_FQ, 5, 3
    m = MOD[field]
    pp, c = public_params_custom(ctx, FC(t, field), field=field), FC(t, field)
    rb, n_cons, _ = pp.repeat_rows()
    z0, traces = z0_of(field), step_traces(field, t, steps)
    proof = None
    for g in (0, 1):                                   # the base step and a step that folds
        c.advice = traces[g]
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
        assert proof.last_unsat() == (0, NONE)
        assert proof.last_unsat() == (0, NONE)         # asking twice changes nothing
    # one wrong entry: x of entry 3.  Repetition j allocates x_(j+1) from entry j + 1 and enforces x_(j+1)^5 = x_j + y_j, where the
    # carries are linear combinations: x_j is the variable of repetition j - 1 and y_j = x_(j-1) + i_in + j - 1 (z_in for j = 0).
    # Which rows fail is computed from that: the wrong x is allocated in repetition 2 and read by repetitions 3 and 4
    e = list(minroot_chain(field, t, steps)[2 * 2 * t:2 * (3 * t + 1)])
    e[2 * 3] = (e[2 * 3] + 1) % m
    xs, i_in = e[0::2], I0 + 2 * t
    ys = [e[1]] + [(xs[j - 1] + i_in + j - 1) % m for j in range(1, t)]
    failing = [j for j in range(t) if pow(xs[j + 1], 5, m) != (xs[j] + ys[j]) % m]
    assert failing == [2, 3, 4]
    c.advice = mont_rows(e, m)
    proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
    assert proof.last_unsat() == (len(failing), rb + failing[0] * n_cons + ENFORCE_INDEX)
    assert proof.verify(pp, 3, z0, zi_of(field, t, steps)) is False
    assert proof.last_unsat() == (len(failing), rb + failing[0] * n_cons + ENFORCE_INDEX)      # (a verifier's scratch use does not matter)
    proof.free(); pp.free()


def test_last_unsat_of_a_built_in_kind(ctx):
    t, n = 5, 3
    pp = public_params(ctx, t)
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, n, State.from_ints(FIELD_FQ, 0x77, 0, 1))
    proof = None
    for k in range(n):                                 # the later steps run their early rows ahead of the step
        proof = NovaVDFProof.prove_step(pp, proof, circuits, k, z0)
        assert proof.last_unsat() == (0, NONE)
    back = NovaVDFProof.deserialize(pp, proof.serialize())
    with pytest.raises(VdfError) as e:                 # no step of this object's yet
        back.last_unsat()
    assert e.value.code == VDF_ERR_BAD_ARG
    back.free(); proof.free(); circuits.free(); pp.free()
