"""The generated column scans of the device field products without a device: tools/gen_fe_mul.py's check mode, and the integer
model of the schedule it EMITS (a 64-bit wrapping accumulator; hi incremented only where a carry add is emitted; an assertion
at every dropped carry add that its multiply-add did not overflow) against redc(T) of tests/prim_spec.py -- all nine words,
for the three bodies in both fields."""
import random
import subprocess
import sys

import numpy as np
import pytest

import fe_scan_cases as c
import prim_spec as s

BODIES = pytest.mark.parametrize("body", c.gen.BODIES)
FIELDS = pytest.mark.parametrize("F", s.FIELDS, ids=repr)


def _check(F, body, tuples):
    got, q = c.run_model(F, body, tuples)
    want = [s.redc(F, c.T_of(body, t)) for t in tuples]
    bad = [i for i in range(len(tuples)) if got[i] != want[i]]
    assert not bad, "%s %s: %d of %d differ from redc(T); first: %s -> %x, want %x" % (
        F, body, len(bad), len(tuples), [hex(v) for v in tuples[bad[0]]], got[bad[0]], want[bad[0]])
    return got, q


def test_generator_check_mode_passes():
    r = subprocess.run([sys.executable, c.gen.__file__, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_dropped_carry_adds_per_body():
    """the counts DESIGN 4.1 quotes, and the rule itself: in every column the carry adds start at the first term whose bound
    takes the running bound of the accumulator to 2^64, the first emitted one writes hi, and nothing is emitted before it"""
    assert [c.gen.dropped(b) for b in c.gen.BODIES] == [31, 38, 31]
    for body in c.gen.BODIES:
        cols = c.gen.schedule(body)
        ref = c.gen.schedule(body, carry_all=True)
        for col, old in zip(cols, ref):
            assert sorted(map(repr, col.terms)) == sorted(map(repr, old.terms))          # the same terms, another order
            assert all(t.carry for t in old.terms)
            assert [t.bound for t in col.terms] == sorted(t.bound for t in col.terms)
            run, seen = col.entry, False
            for t in col.terms:
                run += t.bound
                seen = seen or run >= 1 << 64
                assert bool(t.carry) == seen
            kinds = [t.carry for t in col.terms if t.carry]
            assert kinds == ["first"] + ["acc"] * (len(kinds) - 1) if kinds else not col.has_hi
            assert run == col.total


@BODIES
@FIELDS
def test_model_equals_redc_on_random_operands(F, body):
    """102,400 tuples: [0, m), [m, 2m), [2m, 2m + 9 eps) and uniformly random 256-bit words, a quarter each"""
    rng = random.Random(1000 + 10 * F.fid + c.gen.BODIES.index(body))
    _check(F, body, c.random_operands(F, body, 25600, rng))


@BODIES
@FIELDS
def test_model_equals_redc_on_crafted_operands(F, body):
    """all-ones limbs, top limbs around 2^31 and the lazy domain's edge, and operands that make EVERY quotient digit 0xFFFFFFFF
    (every reduction product at its maximum at once) or every one 0 -- the model's own q digits are checked to be that"""
    tuples, n_edge, n_full = c.adversarial(F, body, 1000)
    assert (c.ONES,) * c.ARITY[body] in tuples
    _, q = _check(F, body, tuples)
    q = np.stack(q, axis=1)
    assert (q[n_edge:n_edge + n_full] == 0xFFFFFFFF).all() and n_full >= 4
    assert (q[n_edge + n_full:] == 0).all() and len(tuples) - n_edge - n_full >= 4


@BODIES
def test_schedule_with_every_carry_add_gives_the_same_words(body):
    """the VDF_FE_CARRY_ALL bodies (the schedule before the bound argument) through the same model: identical words"""
    F = s.FIELDS[0]
    tuples = c.adversarial(F, body, 300)[0] + c.random_operands(F, body, 256, random.Random(5))
    assert c.run_model(F, body, tuples, carry_all=True)[0] == c.run_model(F, body, tuples)[0]


def test_model_trips_on_a_carry_add_dropped_too_early():
    """the assertion at a dropped carry add is live: with the carry adds of column 8 of the product removed, all-ones
    operands (seven products of (2^32 - 1)^2) overflow the accumulator there and the model says so"""
    F = s.FIELDS[0]
    cols = c.gen.schedule("mul")
    for t in cols[8].terms:
        t.carry = None
    ops = [c.to_limbs([c.ONES])] * 2
    with pytest.raises(AssertionError, match="column 8"):
        c.gen.model(cols, c.gen.model_inputs("mul", F.name, *ops))
