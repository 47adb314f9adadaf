"""The generated column scans on the device: fe_mul_inl, fe_mul_lazy, fe_sqr_lazy and fe_mul2_lazy in both fields on the
operand lists of tests/fe_scan_cases.py (all-ones limbs, top limbs around 2^31, every quotient digit 0xFFFFFFFF at once, every
one 0), through tools/ubench/prim_check, bit for bit against the integer semantics.  The lists leave the entry points'
contracts on purpose -- the scans assume nothing beyond 256 bits -- so the expected words are those of the eight-word scan
(tests/fe_scan_cases.py: dev_*), which inside the contracts is tests/prim_spec.py's model.  One child process per field."""
import random

import pytest

import fe_scan_cases as c
import prim_spec as s

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("F", s.FIELDS, ids=repr)
def test_scans_bit_for_bit_on_crafted_operands(F):
    rng = random.Random(77 + F.fid)
    jobs = [(F, op, c.adversarial(F, body, 1000)[0] + c.random_operands(F, body, 64, rng)) for op, (body, _) in c.DEVICE_OPS.items()]
    # inside the entry points' contracts the eight-word semantics are tests/prim_spec.py's
    m = F.m
    assert c.dev_mul_inl(F, m - 1, m - 2) == s.fe_mul_inl(F, m - 1, m - 2)
    assert c.dev_mul2_lazy(F, 2 * m, 2 * m, m + 5, 2 * m - 1) == s.fe_mul2_lazy(F, 2 * m, 2 * m, m + 5, 2 * m - 1)
    res = s.run_jobs(jobs)
    for (_, op, rows), got in zip(jobs, res):
        model = c.DEVICE_OPS[op][1]
        want = [(model(F, *t),) for t in rows]
        bad = [i for i in range(len(rows)) if got[i] != want[i]]
        assert len(rows) >= 1000
        assert not bad, "%s %s: %d of %d cases differ; first: operands %s -> got %s, want %s" % (
            F, op, len(bad), len(rows), [hex(v) for v in rows[bad[0]]], [hex(v) for v in got[bad[0]]], [hex(v) for v in want[bad[0]]])
