"""CPU: the host side of the device random oracle (include/vdf_nova.h) -- vdf_nova_ro_constants and
vdf_nova_ro_hash_batch_eval, the host restatement of vdf_ro_hash_batch that the GPU tests compare with byte for byte.  The
reference is oracle/poseidon.py alone: round_constants for the constants, hash_elements for the hashes, the truncation as
a mask of the canonical integer."""
import os
import random
import re

import numpy as np
import pytest

from oracle import pasta as o, poseidon
from util import ints, limbs, mont
from vdf_amd import nova
from vdf_amd.hip import VdfError
from vdf_amd.minroot import FIELD_FP, FIELD_FQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [FIELD_FP, FIELD_FQ]
LENS = [0, 1, 2, 3, 4, 6, 7, 13, 16, 17]
BITS = [0, 1, 128, 250, 255]
BAD_ARG = 1


def oracle_constants(field):
    """the 88 constants in the order of the C ABI: ext[r][lane] for the 8 external rounds, then the 56 internal ones"""
    rows = poseidon.round_constants(field)
    ext = [v for row in rows if len(row) == 4 for v in row]
    inner = [row[0] for row in rows if len(row) == 1]
    assert len(ext) == 32 and len(inner) == 56
    return ext + inner


def messages(field, ln, n, seed):
    """n messages of ln canonical integers: all zero, all one, all m - 1, one special element per position, then random ones"""
    m = o.modulus(field)
    rng = random.Random(seed)
    out = [[0] * ln, [1] * ln, [m - 1] * ln]
    for j in range(ln):
        out.append([m - 1 if k == j else 0 for k in range(ln)])
    while len(out) < n:
        out.append([rng.choice((0, 1, m - 1, rng.randrange(m), rng.randrange(m))) for _ in range(ln)])
    return out[:n]


def expected(field, tag, msgs, bits):
    m = o.modulus(field)
    hs = [poseidon.hash_elements(tag, msg, field) for msg in msgs]
    return limbs([o.to_mont(h, m) if bits == 0 else h & ((1 << bits) - 1) for h in hs])


def pack(field, msgs):
    m = o.modulus(field)
    return mont([v for msg in msgs for v in msg], m).reshape(-1, 4)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_constants_are_the_oracles_in_the_stated_order(field):
    got = nova.ro_constants(field)
    assert got.shape == (88, 4)
    assert np.array_equal(got, mont(oracle_constants(field), o.modulus(field)))


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("ln", LENS)
def test_batch_eval_against_the_oracle(field, ln):
    n = 3 + ln + 4
    msgs = messages(field, ln, n, 100 * ln + field)
    xs = pack(field, msgs)
    for tag in (1, 2):
        for bits in BITS:
            out = np.full((n + 1, 4), 0xA5A5A5A5A5A5A5A5, dtype="<u8")
            nova.ro_hash_batch_eval(field, tag, xs, ln, n, bits, out)
            assert np.array_equal(out[:n], expected(field, tag, msgs, bits)), (tag, bits)
            assert (out[n] == 0xA5A5A5A5A5A5A5A5).all()                       # n entries written, entry n untouched
    # bits = 0 is vdf_nova_ro_hash's own value
    out = np.zeros((n, 4), dtype="<u8")
    nova.ro_hash_batch_eval(field, 7, xs, ln, n, 0, out)
    for i in range(n):
        assert np.array_equal(out[i], nova.ro_hash(field, 7, xs[i * ln:(i + 1) * ln])), i
    if ln == 0:
        assert not out.any()                                                  # nothing is permuted: lane 1 is still 0


def test_a_tag_whose_sum_with_the_length_carries():
    field, ln = FIELD_FQ, 5
    msgs = messages(field, ln, 6, 9)
    tag = (1 << 33) + 0xFFFFFFFF                                              # tag + (5 << 32) carries out of bit 32
    out = np.zeros((6, 4), dtype="<u8")
    nova.ro_hash_batch_eval(field, tag, pack(field, msgs), ln, 6, 250, out)
    assert np.array_equal(out, expected(field, tag, msgs, 250))


def test_refusals():
    xs = pack(FIELD_FP, messages(FIELD_FP, 3, 2, 1))
    out = np.full((2, 4), 0xA5A5A5A5A5A5A5A5, dtype="<u8")
    calls = {
        "bits = -1": lambda: nova.ro_hash_batch_eval(FIELD_FP, 1, xs, 3, 2, -1, out),
        "bits = 256": lambda: nova.ro_hash_batch_eval(FIELD_FP, 1, xs, 3, 2, 256, out),
        "a bad field": lambda: nova.ro_hash_batch_eval(7, 1, xs, 3, 2, 0, out),
        "len = 1025": lambda: nova.ro_hash_batch_eval(FIELD_FP, 1, np.zeros((2 * 1025, 4), dtype="<u8"), 1025, 2, 0, out),
        "null xs": lambda: nova.ro_hash_batch_eval(FIELD_FP, 1, None, 3, 2, 0, out),
        "null out": lambda: nova.ro_hash_batch_eval(FIELD_FP, 1, xs, 3, 2, 0, None),
    }
    for name, call in calls.items():
        with pytest.raises(VdfError) as e:
            call()
        assert e.value.code == BAD_ARG, name
    assert (out == 0xA5A5A5A5A5A5A5A5).all()                                  # a refused call wrote nothing
    with pytest.raises(VdfError) as e:
        nova.ro_constants(7)
    assert e.value.code == BAD_ARG
    nova.ro_hash_batch_eval(FIELD_FP, 1, None, 3, 0, 0, None)                 # n = 0: VDF_OK, nothing touched
    nova.ro_hash_batch_eval(FIELD_FP, 1, None, 0, 2, 0, out)                  # xs may be null when len = 0
    assert not out.any()
    big = np.zeros((1024, 4), dtype="<u8")                                    # the cap itself is taken
    nova.ro_hash_batch_eval(FIELD_FP, 1, big, 1024, 1, 0, out)
    assert ints(out[:1]) == [o.to_mont(poseidon.hash_elements(1, [0] * 1024, FIELD_FP), o.P)]


def test_both_headers_declare_the_new_calls():
    with open(os.path.join(ROOT, "include", "vdf_hip.h")) as f:
        hip = f.read()
    with open(os.path.join(ROOT, "include", "vdf_nova.h")) as f:
        nv = f.read()
    assert re.search(r"#define\s+VDF_RO_CONSTANTS\s+88\b", hip) and re.search(r"#define\s+VDF_RO_HASH_MAX_LEN\s+1024\b", hip)
    assert re.search(r"\bint\s+vdf_ro_hash_batch\(vdf_ctx\* ctx, int field, uint64_t tag, const vdf_fe\* rc,", hip)
    for name in ("vdf_nova_ro_constants", "vdf_nova_ro_hash_batch_eval", "vdf_nova_pp_set_verify_ro_device", "vdf_nova_pp_verify_ro_device",
                 "vdf_nova_pp_verify_ro_stats"):
        assert re.search(r"\bint\s+" + name + r"\(", nv), name
