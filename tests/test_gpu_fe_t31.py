"""The bounded-top column scans on the device: fe_mul_lazy_t31, fe_sqr_lazy_t31 and fe_mul2_lazy_t31 in both fields on the operand
lists of tests/fe_t31_cases.py (every operand with limb 7 <= 0x80000000: the edges of that range crossed, every quotient digit
0xFFFFFFFF at once, every one 0, random words), through tools/ubench/prim_check, bit for bit against the eight-word
semantics of tests/fe_scan_cases.py -- the very words the generic bodies give.  One child process per field."""
import random

import pytest

import fe_scan_cases as c
import fe_t31_cases as t31
import prim_spec as s

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("F", s.FIELDS, ids=repr)
def test_bounded_scans_bit_for_bit_on_crafted_operands(F):
    rng = random.Random(91 + F.fid)
    jobs = []
    for op, (_, _, _, body, _) in t31.T31_OPS.items():
        rows = t31.adversarial(F, body, 1000)[0] + t31.random_operands(F, body, 64, rng)
        assert len(rows) >= 1000
        jobs.append((F, op, rows))
    res = t31.run_jobs(jobs)
    for (_, op, rows), got in zip(jobs, res):
        model = t31.T31_OPS[op][4]
        want = [(model(F, *t),) for t in rows]
        bad = [i for i in range(len(rows)) if got[i] != want[i]]
        assert not bad, "%s %s: %d of %d cases differ; first: operands %s -> got %s, want %s" % (
            F, op, len(bad), len(rows), [hex(v) for v in rows[bad[0]]], [hex(v) for v in got[bad[0]]], [hex(v) for v in want[bad[0]]])
