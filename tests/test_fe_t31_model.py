"""The bounded-top column scans (fe_{mul,sqr,mul2}_t31_gfx950.inc) without a device: the integer model of the schedule
tools/gen_fe_mul.py EMITS for multiplicands whose limb 7 is at most 2^31 (an assertion at every dropped carry add) against
redc(T) of tests/prim_spec.py, all nine words, three bodies, both fields -- and the precondition itself: that it is needed
(operands above it trip the model), and that every factor the two lazy additions of ec.cuh hand to a product satisfies it."""
import random

import numpy as np
import pytest

import fe_scan_cases as c
import fe_t31_cases as t31
import prim_spec as s

o = s.o
BODIES = pytest.mark.parametrize("body", c.gen.BODIES)
FIELDS = pytest.mark.parametrize("F", s.FIELDS, ids=repr)


def _check(F, body, tuples):
    assert all(t31.bounded(v) for t in tuples for v in t)
    got, q = t31.run_model(F, body, tuples)
    want = [s.redc(F, c.T_of(body, t)) for t in tuples]
    bad = [i for i in range(len(tuples)) if got[i] != want[i]]
    assert not bad, "%s %s: %d of %d differ from redc(T); first: %s -> %x, want %x" % (
        F, body, len(bad), len(tuples), [hex(v) for v in tuples[bad[0]]], got[bad[0]], want[bad[0]])
    return got, q


def test_dropped_carry_adds_of_the_bounded_bodies():
    """39 / 39 / 40 (31 / 38 / 31 without the bound), by the same rule: within a column the carry adds start at the first term
    that takes the running bound of the accumulator to 2^64.  The order is ascending within each asm statement (the second
    product of the pair has a statement of its own, behind the first's), and only limb 7 of a multiplicand has the new bound"""
    assert [c.gen.dropped(b, top31=True) for b in c.gen.BODIES] == [39, 39, 40]
    assert [c.gen.dropped(b) for b in c.gen.BODIES] == [31, 38, 31]
    for body in c.gen.BODIES:
        for col, old in zip(c.gen.schedule(body, top31=True), c.gen.schedule(body, carry_all=True)):
            assert sorted(map(repr, col.terms)) == sorted(map(repr, old.terms))
            assert [t.second for t in col.terms] == sorted(t.second for t in col.terms)
            for stmt in (False, True):
                b = [t.bound for t in col.terms if t.second == stmt]
                assert b == sorted(b)
            run, seen = col.entry, False
            for t in col.terms:
                narrow = [n for n in (t.x, t.y) if n in (("a7",) if body == "sqr" else ("a7", "b7", "c7", "d7"))]
                assert t.bound == c.gen.bound(body, t.x, True) * c.gen.bound(body, t.y, True)
                assert (c.gen.bound(body, t.x, True) == 1 << 31) == (t.x in narrow) and (c.gen.bound(body, t.y, True) == 1 << 31) == (t.y in narrow)
                run += t.bound
                seen = seen or run >= 1 << 64
                assert bool(t.carry) == seen
            kinds = [t.carry for t in col.terms if t.carry]
            assert kinds == ["first"] + ["acc"] * (len(kinds) - 1) if kinds else not col.has_hi
            assert run == col.total


@BODIES
@FIELDS
def test_bounded_model_equals_redc_on_random_operands(F, body):
    """100,000 tuples: [0, m), [m, 2m), [2m, 2m + 9 eps) and uniformly random words with limb 7 <= 2^31, a quarter each"""
    rng = random.Random(3100 + 10 * F.fid + c.gen.BODIES.index(body))
    tuples = t31.random_operands(F, body, 25000, rng)
    assert len(tuples) == 100000
    _check(F, body, tuples)


@BODIES
@FIELDS
def test_bounded_model_equals_redc_on_crafted_operands(F, body):
    """the edge operands inside the precondition (limb 7 = 0x80000000 over all-ones lower limbs among them), crossed; every
    quotient digit 0xFFFFFFFF at once with bounded factors, and every one 0 -- the model's own digits are checked to be that"""
    tuples, n_edge, n_full = t31.adversarial(F, body, 1000)
    top = (t31.TOP << 224) | ((1 << 224) - 1)
    assert (top,) * c.ARITY[body] in tuples
    _, q = _check(F, body, tuples)
    q = np.stack(q, axis=1)
    assert (q[n_edge:n_edge + n_full] == 0xFFFFFFFF).all() and n_full >= (2 if body == "sqr" else 1000)
    assert (q[n_edge + n_full:] == 0).all() and len(tuples) - n_edge - n_full >= 1000


def test_bounded_product_needs_its_precondition():
    """operands of the generic lists with a top limb above 2^31 overflow the accumulator at a carry add only the bound let go"""
    F = s.FIELDS[0]
    tuples = [t for t in c.adversarial(F, "mul", 1000)[0] if not all(map(t31.bounded, t))]
    assert tuples
    tripped = 0
    for t in tuples[:200]:
        try:
            t31.run_model(F, "mul", [t])
        except AssertionError as e:
            assert "overflowed the accumulator with its carry add dropped" in str(e)
            tripped += 1
    assert tripped >= 1
    with pytest.raises(AssertionError, match="carry add dropped"):
        t31.run_model(F, "mul", [(c.ONES, c.ONES)])
    c.run_model(F, "mul", tuples)                                     # the generic schedule takes them all


class _Watch:
    """prim_spec's three lazy products with every factor checked against the bounded bodies' precondition"""
    def __init__(self, monkeypatch):
        self.calls = 0
        for name in ("fe_mul_lazy", "fe_sqr_lazy", "fe_mul2_lazy"):
            monkeypatch.setattr(s, name, self._wrap(name, getattr(s, name)))

    def _wrap(self, name, fn):
        def checked(F, *ops):
            for v in ops:
                assert t31.bounded(v), "%s: factor %x has limb 7 above 2^31" % (name, v)
            self.calls += 1
            return fn(F, *ops)
        return checked


@FIELDS
@pytest.mark.parametrize("lazy_add", (False, True), ids=("madd", "add"))
def test_every_factor_of_the_lazy_additions_is_bounded_on_the_crafted_states(F, lazy_add, monkeypatch):
    w = _Watch(monkeypatch)
    cases = s.lazy_cases(F, lazy_add)                                 # runs every state through the (watched) model itself
    for case in cases:
        s.lazy_model_row(F, lazy_add, case)
    assert w.calls > 10 * len(cases)


@FIELDS
def test_every_factor_of_the_lazy_additions_is_bounded_along_chains(F, monkeypatch):
    """3,000 mixed additions and 2,000 full ones, as the bucket loop and the serial fix-up run them (the addend negated for a
    pending sign), over a small pool with repeats and negatives: doublings, cancellations and restarts on the way.  Every
    factor is inside the precondition, every stored accumulator inside its slack, and the sum is the oracle's"""
    w = _Watch(monkeypatch)
    m = F.m
    rng = random.Random(4100 + F.fid)
    pool = [s.mul_g(F, rng.randrange(2, 1 << 24)) for _ in range(6)]
    pool += [o.pt_neg(p, m) for p in pool]
    for lazy_add, steps, slack2 in ((False, 3000, s.MADD_SLACK2), (True, 2000, s.ADD_SLACK2)):
        step = s.xyzz_add_lazy if lazy_add else s.xyzz_madd_lazy
        acc, have, flip, total, events = (0, 0, 0, 0), 0, 0, None, set()
        for i in range(steps):
            # now and then the accumulator's own point or its negative: a doubling or a cancellation
            B = total if (i % 97 == 50 and total) else o.pt_neg(total, m) if (i % 97 == 75 and total) else rng.choice(pool)
            b = list(s.xyzz_mont(F, B, rng.randrange(1, m)) if lazy_add else s.affine_mont(F, B))
            if have and flip:
                b[1] = s.fe_neg_nz(F, b[1])
            had = have
            acc, have, flip, Pn = step(F, acc, have, flip, tuple(b))
            total = o.pt_add(total, B, m)
            events.add("first" if not had else "gone" if not have else "same_x" if Pn % m == 0 else "general")
            assert not have or s.inside(F, acc, slack2)
            assert s.xyzz_point(F, tuple(s.fe_canon(F, v) for v in s.xyzz_lazy_resolve(F, acc, have, flip))) == total
        assert events == {"first", "gone", "same_x", "general"}
    assert w.calls > 40000
