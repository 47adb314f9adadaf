"""CPU: the host side of the family-1 device random oracle (include/vdf_nova.h) -- vdf_nova_ro_block_constants, the constants
vdf_ro_hash_batch_block reads, and vdf_nova_ro_hash_batch_eval_ro, the host restatement the GPU tests compare with byte for
byte.  The reference is oracle/poseidon.py alone: classic_constants for the constants, hash_elements under using(spec) for
the hashes, the truncation as a mask of the canonical integer."""
import os
import random
import re

import numpy as np
import pytest

from oracle import pasta as o, poseidon
from util import limbs, mont
from vdf_amd import nova
from vdf_amd.hip import VdfError
from vdf_amd.minroot import FIELD_FP, FIELD_FQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [FIELD_FP, FIELD_FQ]
SMALL = poseidon.RoSpec(family=1, width=9, full_rounds=8, partial_rounds=30)           # the small instance of tests/test_nova_host.py
WIDTH_2 = poseidon.RoSpec(family=1, width=2, full_rounds=2, partial_rounds=0)
SPECS = {"width 9": SMALL, "neptune-shaped": poseidon.NEPTUNE_SHAPED, "width 2": WIDTH_2}
BITS = [0, 1, 128, 250, 255]
BAD_ARG = 1
FILL = 0xA5A5A5A5A5A5A5A5


def block(spec):
    """the ABI's parameter block of an oracle RoSpec"""
    which = nova.RO_NEPTUNE_SHAPED if spec.family == 1 else nova.RO_DEFAULT
    return nova.ro_preset(which, width=spec.width, full_rounds=spec.full_rounds, partial_rounds=spec.partial_rounds)


def messages(field, ln, n, seed):
    """n messages of ln canonical integers: all zero, all m - 1, one non-zero element per position (the first six), then
    elements drawn from {0, 1, m - 1, random}"""
    m = o.modulus(field)
    rng = random.Random(seed)
    out = [[0] * ln, [m - 1] * ln]
    for j in range(min(ln, 6)):
        out.append([rng.randrange(1, m) if k == j else 0 for k in range(ln)])
    while len(out) < n:
        out.append([rng.choice((0, 1, m - 1, rng.randrange(m), rng.randrange(m))) for _ in range(ln)])
    return out[:n]


def hashes(spec, field, tag, msgs):
    with poseidon.using(spec):
        return [poseidon.hash_elements(tag, msg, field) for msg in msgs]


def truncated(field, hs, bits):
    m = o.modulus(field)
    return limbs([o.to_mont(h, m) if bits == 0 else h & ((1 << bits) - 1) for h in hs])


def expected(spec, field, tag, msgs, bits):
    return truncated(field, hashes(spec, field, tag, msgs), bits)


def pack(field, msgs):
    return mont([v for msg in msgs for v in msg], o.modulus(field)).reshape(-1, 4)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("name", SPECS)
def test_constants_are_the_oracles_in_the_stated_layout(field, name):
    spec = SPECS[name]
    m = o.modulus(field)
    rc, mds = nova.ro_block_constants(field, block(spec))
    want_rc, want_mds = poseidon.classic_constants(field, spec)
    t, rounds = spec.width, spec.full_rounds + spec.partial_rounds
    assert rc.shape == (rounds * t, 4) and mds.shape == (t * t, 4)
    assert np.array_equal(rc, mont([v for row in want_rc for v in row], m).reshape(-1, 4))        # round-major, lane-minor
    assert np.array_equal(mds, mont([v for row in want_mds for v in row], m).reshape(-1, 4))      # row-major


def test_the_counts_call_and_partial_requests():
    import ctypes as C
    ro = block(poseidon.NEPTUNE_SHAPED)
    counts = (C.c_size_t * 2)()
    assert nova.nova_lib.vdf_nova_ro_block_constants(C.byref(ro), FIELD_FQ, None, None, counts) == 0
    assert list(counts) == [65 * 25, 625]
    rc, mds = nova.ro_block_constants(FIELD_FQ, ro)
    only_rc = np.zeros_like(rc)
    assert nova.nova_lib.vdf_nova_ro_block_constants(C.byref(ro), FIELD_FQ, only_rc.ctypes.data, None, None) == 0
    assert np.array_equal(only_rc, rc)
    only_mds = np.zeros_like(mds)
    assert nova.nova_lib.vdf_nova_ro_block_constants(C.byref(ro), FIELD_FQ, None, only_mds.ctypes.data, None) == 0
    assert np.array_equal(only_mds, mds)


def test_constants_refusals():
    import ctypes as C
    counts = (C.c_size_t * 2)()
    assert nova.nova_lib.vdf_nova_ro_block_constants(None, FIELD_FP, None, None, counts) == BAD_ARG              # ro = NULL
    for ro in (nova.ro_preset(nova.RO_DEFAULT),                                    # family 0 has vdf_nova_ro_constants
               nova.ro_preset(nova.RO_NEPTUNE_SHAPED, width=26), nova.ro_preset(nova.RO_NEPTUNE_SHAPED, width=1),
               nova.ro_preset(nova.RO_NEPTUNE_SHAPED, full_rounds=7), nova.ro_preset(nova.RO_NEPTUNE_SHAPED, partial_rounds=129)):
        with pytest.raises(VdfError) as e:
            nova.ro_block_constants(FIELD_FP, ro)
        assert e.value.code == BAD_ARG, ro.as_dict()
    with pytest.raises(VdfError) as e:
        nova.ro_block_constants(7, block(SMALL))
    assert e.value.code == BAD_ARG
    assert list(counts) == [0, 0]


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("name", SPECS)
def test_batch_eval_against_the_oracle(field, name):
    spec = SPECS[name]
    ro, rate = block(spec), spec.width - 1
    n = 5
    for ln in sorted({0, 1, rate - 1, rate, rate + 1, 2 * rate + 1}):
        msgs = messages(field, ln, n, 100 * ln + field)
        xs = pack(field, msgs)
        hs = hashes(spec, field, 1, msgs)
        for bits in BITS:
            out = np.full((n + 1, 4), FILL, dtype="<u8")
            nova.ro_hash_batch_eval(field, 1, xs, ln, n, bits, out, ro=ro)
            assert np.array_equal(out[:n], truncated(field, hs, bits)), (ln, bits)
            assert (out[n] == FILL).all()                                         # n entries written, entry n untouched
        out = np.zeros((n, 4), dtype="<u8")                                       # bits = 0 is vdf_nova_ro_hash_ro's own value
        nova.ro_hash_batch_eval(field, 2, xs, ln, n, 0, out, ro=ro)
        for i in range(n):
            assert np.array_equal(out[i], nova.ro_hash(field, 2, xs[i * ln:(i + 1) * ln], ro)), (ln, i)
        if ln == 0:
            assert not out.any()                                                  # nothing is permuted: element 1 is still 0


def test_a_tag_whose_sum_with_the_length_carries():
    field, ln = FIELD_FQ, 5
    msgs = messages(field, ln, 4, 9)
    tag = (1 << 33) + 0xFFFFFFFF                                                  # tag + (5 << 32) carries out of bit 32
    out = np.zeros((4, 4), dtype="<u8")
    nova.ro_hash_batch_eval(field, tag, pack(field, msgs), ln, 4, 250, out, ro=block(SMALL))
    assert np.array_equal(out, expected(SMALL, field, tag, msgs, 250))


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_a_null_block_is_the_default_blocks_call(field):
    import ctypes as C
    for ln in (0, 4, 7):
        msgs = messages(field, ln, 6, ln)
        xs = pack(field, msgs)
        for bits in (0, 128, 250):
            a, b, c = (np.full((6, 4), FILL, dtype="<u8") for _ in range(3))
            nova.ro_hash_batch_eval(field, 1, xs, ln, 6, bits, a)
            assert nova.nova_lib.vdf_nova_ro_hash_batch_eval_ro(None, field, 1, xs.ctypes.data, ln, 6, bits, b.ctypes.data) == 0
            nova.ro_hash_batch_eval(field, 1, xs, ln, 6, bits, c, ro=nova.ro_preset(nova.RO_DEFAULT))
            assert np.array_equal(a, b) and np.array_equal(a, c) and not (a == FILL).all()
            assert np.array_equal(a, expected(poseidon.DEFAULT, field, 1, msgs, bits))


def test_refusals():
    ro = block(SMALL)
    xs = pack(FIELD_FP, messages(FIELD_FP, 3, 2, 1))
    out = np.full((2, 4), FILL, dtype="<u8")
    hash_ = lambda field, xs_, ln, n, bits, out_, ro_=ro: nova.ro_hash_batch_eval(field, 1, xs_, ln, n, bits, out_, ro=ro_)
    calls = {
        "a bad field": lambda: hash_(7, xs, 3, 2, 0, out),
        "width = 26": lambda: hash_(FIELD_FP, xs, 3, 2, 0, out, nova.ro_preset(nova.RO_NEPTUNE_SHAPED, width=26)),
        "width = 1": lambda: hash_(FIELD_FP, xs, 3, 2, 0, out, nova.ro_preset(nova.RO_NEPTUNE_SHAPED, width=1)),
        "full_rounds = 3": lambda: hash_(FIELD_FP, xs, 3, 2, 0, out, nova.ro_preset(nova.RO_NEPTUNE_SHAPED, full_rounds=3)),
        "full_rounds = 18": lambda: hash_(FIELD_FP, xs, 3, 2, 0, out, nova.ro_preset(nova.RO_NEPTUNE_SHAPED, full_rounds=18)),
        "partial_rounds = 129": lambda: hash_(FIELD_FP, xs, 3, 2, 0, out, nova.ro_preset(nova.RO_NEPTUNE_SHAPED, partial_rounds=129)),
        "partial_rounds = -1": lambda: hash_(FIELD_FP, xs, 3, 2, 0, out, nova.ro_preset(nova.RO_NEPTUNE_SHAPED, partial_rounds=-1)),
        "bits = -1": lambda: hash_(FIELD_FP, xs, 3, 2, -1, out),
        "bits = 256": lambda: hash_(FIELD_FP, xs, 3, 2, 256, out),
        "len = 1025": lambda: hash_(FIELD_FP, np.zeros((2 * 1025, 4), dtype="<u8"), 1025, 2, 0, out),
        "null xs": lambda: hash_(FIELD_FP, None, 3, 2, 0, out),
        "null out": lambda: hash_(FIELD_FP, xs, 3, 2, 0, None),
    }
    for name, call in calls.items():
        with pytest.raises(VdfError) as e:
            call()
        assert e.value.code == BAD_ARG, name
    assert (out == FILL).all()                                                    # a refused call wrote nothing
    hash_(FIELD_FP, None, 3, 0, 0, None)                                          # n = 0: VDF_OK, nothing touched
    hash_(FIELD_FP, None, 0, 2, 0, out)                                           # xs may be null when len = 0
    assert not out.any()
    big = np.zeros((1024, 4), dtype="<u8")                                        # the cap itself is taken
    hash_(FIELD_FP, big, 1024, 1, 0, out, block(WIDTH_2))
    assert np.array_equal(out[:1], expected(WIDTH_2, FIELD_FP, 1, [[0] * 1024], 0))


def test_both_headers_declare_the_new_calls():
    with open(os.path.join(ROOT, "include", "vdf_hip.h")) as f:
        hip = f.read()
    with open(os.path.join(ROOT, "include", "vdf_nova.h")) as f:
        nv = f.read()
    for name, value in (("VDF_RO_BLOCK_MAX_WIDTH", 25), ("VDF_RO_BLOCK_MAX_FULL", 16), ("VDF_RO_BLOCK_MAX_PARTIAL", 128)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", hip), name
    assert re.search(r"\bint\s+vdf_ro_hash_batch_block\(vdf_ctx\* ctx, int field, uint64_t tag, int width, int full_rounds, int partial_rounds,", hip)
    for name in ("vdf_nova_ro_block_constants", "vdf_nova_ro_hash_batch_eval_ro", "vdf_nova_pp_set_verify_ro_block_device",
                 "vdf_nova_pp_verify_ro_block_device"):
        assert re.search(r"\bint\s+" + name + r"\(", nv), name
