"""GPU: vdf_ro_hash_batch (include/vdf_hip.h) -- the family-0 random oracle, one lane per message, the per-entry hashes of the
aggregate's device verifier.  Every output is compared byte for byte with vdf_nova_ro_hash_batch_eval, the host restatement
(tests/test_ro_batch_host.py holds that one to oracle/poseidon.py); the first four messages of every pool are checked against
oracle/poseidon.py directly as well.  Outputs are pre-filled, and one entry more than n is allocated, so that an unwritten or
an over-written entry shows."""
import random

import numpy as np
import pytest

from oracle import pasta as o, poseidon
from util import limbs, mont
from vdf_amd import nova
from vdf_amd.hip import VdfError
from vdf_amd.minroot import FIELD_FP, FIELD_FQ

pytestmark = pytest.mark.gpu
FIELDS = [FIELD_FP, FIELD_FQ]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]               # wave and workgroup edges, and four workgroups
LENS = [0, 1, 2, 3, 4, 5, 6, 7, 13, 16, 17, 107, 1024]     # 107: sixteen lanes' state hash; 1024: the cap
BITS = [0, 1, 128, 250, 255]
FILL = 0xA5A5A5A5A5A5A5A5
TAG_STATE, TAG_CHAL = 1, 2
BAD_ARG = 1
_POOLS, _RC = {}, {}


def rc(field):
    if field not in _RC:
        _RC[field] = nova.ro_constants(field)
        _RC[field].setflags(write=False)
    return _RC[field]


def pool(field, ln, n):
    """n messages of ln elements (uint64[n * ln, 4], Montgomery form), made once and never changed: all zero, all m - 1, one
    non-zero element in each position of the first two blocks, then elements drawn from {0, 1, m - 1, random}"""
    key = (field, ln, n)
    if key not in _POOLS:
        m = o.modulus(field)
        rng = random.Random(0x50 + 1000 * ln + field)
        msgs = [[0] * ln, [m - 1] * ln]
        for j in range(min(ln, 6)):
            msgs.append([rng.randrange(1, m) if k == j else 0 for k in range(ln)])
        while len(msgs) < n:
            msgs.append([rng.choice((0, 1, m - 1, rng.randrange(m), rng.randrange(m), rng.randrange(m))) for _ in range(ln)])
        msgs = msgs[:n]
        arr = mont([v for msg in msgs for v in msg], m).reshape(-1, 4)
        arr.setflags(write=False)
        _POOLS[key] = (arr, msgs[:4])
    return _POOLS[key]


def reference(field, tag, xs, ln, n, bits):
    want = np.full((n, 4), FILL, dtype="<u8")
    nova.ro_hash_batch_eval(field, tag, xs, ln, n, bits, want)
    return want


def by_the_oracle(field, tag, msgs, bits):
    m = o.modulus(field)
    hs = [poseidon.hash_elements(tag, msg, field) for msg in msgs]
    return limbs([o.to_mont(h, m) if bits == 0 else h & ((1 << bits) - 1) for h in hs])


def _place(arr, on_device):
    if not on_device:
        return arr
    import torch
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()


def _hash(ctx, field, tag, xs, ln, n, bits, placement=(False, False, False)):
    """out uint64[n + 1, 4] of vdf_ro_hash_batch over n messages, pre-filled; row n must come back untouched"""
    out = np.full((n + 1, 4), FILL, dtype="<u8")
    drc, dxs, dout = (_place(np.array(x), p) for x, p in zip((rc(field), xs, out), placement))
    ctx.ro_hash_batch(field, tag, drc, dxs, ln, n, bits, dout)
    ctx.sync()
    return dout if isinstance(dout, np.ndarray) else dout.cpu().numpy().view("<u8").reshape(n + 1, 4)


def check(ctx, field, tag, ln, n, bits, placement=(False, False, False)):
    xs, first = pool(field, ln, n)
    out = _hash(ctx, field, tag, xs, ln, n, bits, placement)
    want = reference(field, tag, xs, ln, n, bits)
    bad = np.nonzero((out[:n] != want).any(axis=1))[0]
    assert bad.size == 0, (field, tag, ln, n, bits, placement, bad[:8])
    assert (out[n] == FILL).all(), "entry n was written"
    assert np.array_equal(out[:len(first)], by_the_oracle(field, tag, first, bits))


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_memory_kinds(ctx, field, n):
    """every size from all-host arrays, all-device arrays and a mixture that changes with the size"""
    k = SIZES.index(n)
    mixed = (bool(k & 1), bool(k & 2), not (k & 1))
    for placement in ((False,) * 3, (True,) * 3, mixed):
        check(ctx, field, TAG_STATE, 17, n, 250, placement)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("ln", LENS)
def test_lengths(ctx, field, ln):
    check(ctx, field, TAG_STATE, ln, 65, 250, (True,) * 3)
    if ln == 0:
        assert not _hash(ctx, field, TAG_STATE, np.zeros((0, 4), dtype="<u8"), 0, 65, 0)[:65].any()   # nothing is permuted: 0


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("bits", BITS)
def test_truncations(ctx, field, bits):
    check(ctx, field, TAG_CHAL, 16, 65, bits)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_tags(ctx, field):
    """two tags, and one above 2^32 whose sum with len << 32 carries out of bit 32"""
    for tag in (TAG_STATE, TAG_CHAL, (1 << 33) + 0xFFFFFFFF):
        check(ctx, field, tag, 7, 65, 0)
    a = _hash(ctx, field, TAG_STATE, pool(field, 7, 65)[0], 7, 65, 0)
    b = _hash(ctx, field, TAG_CHAL, pool(field, 7, 65)[0], 7, 65, 0)
    assert (a[:65] != b[:65]).any(axis=1).all()


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_one_non_zero_element_in_each_position(ctx, field):
    """a wrong lane assignment or a missing permutation after a short last block shows on these"""
    m = o.modulus(field)
    for ln in (1, 2, 3, 4, 5, 6):
        msgs = [[0] * ln, [m - 1] * ln] + [[5 if k == j else 0 for k in range(ln)] for j in range(ln)]
        xs = mont([v for msg in msgs for v in msg], m).reshape(-1, 4)
        out = _hash(ctx, field, TAG_STATE, xs, ln, len(msgs), 0)
        assert np.array_equal(out[:len(msgs)], by_the_oracle(field, TAG_STATE, msgs, 0)), ln
        assert len({bytes(r) for r in out[:len(msgs)]}) == len(msgs)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_host_and_device_pointers_in_each_position(ctx, field):
    for mask in range(8):
        check(ctx, field, TAG_STATE, 13, 65, 250, tuple(bool(mask >> j & 1) for j in range(3)))


def test_nothing_is_touched_for_no_messages(ctx):
    import torch
    out = np.full((2, 4), FILL, dtype="<u8")
    ctx.ro_hash_batch(FIELD_FP, 1, rc(FIELD_FP), np.zeros((0, 4), dtype="<u8"), 3, 0, 250, out)
    ctx.ro_hash_batch(FIELD_FQ, 1, None, None, 3, 0, 0, None)
    assert (out == FILL).all()
    dout = torch.from_numpy(out.view(np.int64).copy()).cuda()
    ctx.ro_hash_batch(FIELD_FP, 1, dout, dout, 3, 0, 128, dout)
    ctx.sync()
    assert (dout.cpu().numpy().view("<u8") == FILL).all()


def test_refusals(ctx):
    """each refusal is followed by one good call: the context goes on working"""
    import torch
    field, ln, n = FIELD_FP, 3, 2
    xs = np.array(pool(field, ln, 65)[0][:ln * n])
    want = reference(field, 1, xs, ln, n, 250)
    out = np.full((n, 4), FILL, dtype="<u8")
    consts = np.array(rc(field))
    buf = torch.zeros(32 * 88 + 32 * ln * n + 64, dtype=torch.uint8, device="cuda")        # misaligned device pointers: 8 bytes off
    buf[8:8 + 32 * 88] = torch.from_numpy(consts.view(np.uint8).reshape(-1).copy()).cuda()
    calls = {
        "bits = -1": lambda: ctx.ro_hash_batch(field, 1, consts, xs, ln, n, -1, out),
        "bits = 256": lambda: ctx.ro_hash_batch(field, 1, consts, xs, ln, n, 256, out),
        "a bad field": lambda: ctx.ro_hash_batch(7, 1, consts, xs, ln, n, 250, out),
        "len = 1025": lambda: ctx.ro_hash_batch(field, 1, consts, np.zeros((1025 * n, 4), dtype="<u8"), 1025, n, 250, out),
        "null rc": lambda: ctx.ro_hash_batch(field, 1, None, xs, ln, n, 250, out),
        "null xs": lambda: ctx.ro_hash_batch(field, 1, consts, None, ln, n, 250, out),
        "null out": lambda: ctx.ro_hash_batch(field, 1, consts, xs, ln, n, 250, None),
        "misaligned device rc": lambda: ctx.ro_hash_batch(field, 1, buf.data_ptr() + 8, xs, ln, n, 250, out),
        "misaligned device xs": lambda: ctx.ro_hash_batch(field, 1, consts, buf.data_ptr() + 8, ln, n, 250, out),
        "misaligned device out": lambda: ctx.ro_hash_batch(field, 1, consts, xs, ln, n, 250, buf.data_ptr() + 8),
    }
    for name, call in calls.items():
        with pytest.raises(VdfError) as e:
            call()
        assert e.value.code == BAD_ARG, name
        assert (out == FILL).all(), name                                       # a refused call wrote nothing
        good = np.full((n, 4), FILL, dtype="<u8")
        ctx.ro_hash_batch(field, 1, consts, xs, ln, n, 250, good)
        assert np.array_equal(good, want), name
    ctx.ro_hash_batch(field, 1, consts, None, 0, n, 0, out)                    # xs may be null when len = 0
    assert not out.any()
