"""GPU: vdf_ro_hash_batch_block (include/vdf_hip.h) -- the family-1 random oracle (dense matrix, width up to 25), one message
per 32 lanes, two messages per wavefront, eight per workgroup.  Every output is compared byte for byte with
vdf_nova_ro_hash_batch_eval_ro, the host restatement (tests/test_ro_block_host.py holds that one to oracle/poseidon.py); the
first four messages of every pool are checked against oracle/poseidon.py directly as well, at every shape (the oracle makes a
shape's constants once per process: a few seconds for width 25 with 16 + 128 rounds, the largest).  Outputs are pre-filled, and
one entry more than n is allocated, so that an unwritten or an over-written entry shows.  Pools, placement and fill are those
of tests/test_gpu_ro_hash.py."""
import numpy as np
import pytest

from oracle import pasta as o, poseidon
from test_gpu_ro_hash import FILL, _place, pool
from util import limbs, mont
from vdf_amd import nova
from vdf_amd.hip import VdfError
from vdf_amd.minroot import FIELD_FP, FIELD_FQ

pytestmark = pytest.mark.gpu
FIELDS = [FIELD_FP, FIELD_FQ]
SIZES = [1, 2, 3, 7, 8, 9, 16, 17, 1000]       # the second message of a wavefront, the workgroup edge at 8, many workgroups
WIDTHS = [2, 3, 9, 24, 25]
ROUNDS = [(2, 0), (8, 30), (8, 57), (16, 128)]
BITS = [0, 1, 128, 250, 255]
MAX_LEN = 1024
BAD_ARG = 1
_CONSTS, _WANT = {}, {}


def spec_of(width, rounds=(8, 57)):
    return poseidon.RoSpec(family=1, width=width, full_rounds=rounds[0], partial_rounds=rounds[1])


NEPTUNE, NARROW = spec_of(25), spec_of(2)
assert NEPTUNE == poseidon.NEPTUNE_SHAPED


def block(spec):
    return nova.ro_preset(nova.RO_NEPTUNE_SHAPED, width=spec.width, full_rounds=spec.full_rounds, partial_rounds=spec.partial_rounds)


def consts(field, spec):
    if (field, spec) not in _CONSTS:
        rc, mds = nova.ro_block_constants(field, block(spec))
        rc.setflags(write=False)
        mds.setflags(write=False)
        _CONSTS[field, spec] = (rc, mds)
    return _CONSTS[field, spec]


def lens_of(spec):
    rate = spec.width - 1
    return sorted({0, 1, rate - 1, rate, rate + 1, 2 * rate, 2 * rate + 1})


def reference(spec, field, tag, xs, ln, n, bits):
    """the restatement's n outputs, computed once per case and never changed"""
    key = (spec, field, tag, ln, n, bits, xs.ctypes.data)
    if key not in _WANT:
        want = np.full((n, 4), FILL, dtype="<u8")
        nova.ro_hash_batch_eval(field, tag, xs, ln, n, bits, want, ro=block(spec))
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def by_the_oracle(spec, field, tag, msgs, bits):
    m = o.modulus(field)
    with poseidon.using(spec):
        hs = [poseidon.hash_elements(tag, msg, field) for msg in msgs]
    return limbs([o.to_mont(h, m) if bits == 0 else h & ((1 << bits) - 1) for h in hs])


def _hash(ctx, spec, field, tag, xs, ln, n, bits, placement=(False,) * 4):
    """out uint64[n + 1, 4] of vdf_ro_hash_batch_block over n messages, pre-filled; row n must come back untouched"""
    out = np.full((n + 1, 4), FILL, dtype="<u8")
    rc, mds = consts(field, spec)
    drc, dmds, dxs, dout = (_place(np.array(x), p) for x, p in zip((rc, mds, xs, out), placement))
    ctx.ro_hash_batch_block(field, tag, spec.width, spec.full_rounds, spec.partial_rounds, drc, dmds, dxs, ln, n, bits, dout)
    ctx.sync()
    return dout if isinstance(dout, np.ndarray) else dout.cpu().numpy().view("<u8").reshape(n + 1, 4)


def check(ctx, spec, field, tag, ln, n, bits, placement=(False,) * 4):
    xs, first = pool(field, ln, n)
    out = _hash(ctx, spec, field, tag, xs, ln, n, bits, placement)
    want = reference(spec, field, tag, xs, ln, n, bits)
    bad = np.nonzero((out[:n] != want).any(axis=1))[0]
    assert bad.size == 0, (spec, field, tag, ln, n, bits, placement, bad[:8])
    assert (out[n] == FILL).all(), "entry n was written"
    assert np.array_equal(out[:len(first)], by_the_oracle(spec, field, tag, first, bits))


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_memory_kinds(ctx, field, n):
    """every size at width 25 and at width 2, from all-host arrays, all-device arrays and a mixture that changes with the size"""
    k = SIZES.index(n)
    mixed = (bool(k & 1), bool(k & 2), bool(k & 4), not (k & 1))
    for placement in ((False,) * 4, (True,) * 4, mixed):
        check(ctx, NEPTUNE, field, 1, 17, n, 250, placement)
        check(ctx, NARROW, field, 1, 3, n, 250, placement)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("width", WIDTHS)
def test_widths(ctx, field, width):
    """lanes >= width idle: one block, a short block and two blocks and a short one at every width"""
    spec = spec_of(width, (8, 30))
    rate = width - 1
    for ln in sorted({rate, rate + 1, 2 * rate + 1}):
        check(ctx, spec, field, 1, ln, 9, 250, (True,) * 4)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("rounds", ROUNDS, ids=lambda r: "%d+%d" % r)
def test_rounds(ctx, field, rounds):
    """no partial rounds, an even and an odd number of rounds (the slots' parity runs on into the next permutation), the caps"""
    for width in (25, 2):
        spec = spec_of(width, rounds)
        check(ctx, spec, field, 2, 2 * (width - 1) + 1, 9, 128, (True,) * 4)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("spec", [NEPTUNE, NARROW], ids=["width 25", "width 2"])
def test_lengths(ctx, field, spec):
    for ln in lens_of(spec):
        check(ctx, spec, field, 1, ln, 9, 250, (True,) * 4)
    assert not _hash(ctx, spec, field, 1, np.zeros((0, 4), dtype="<u8"), 0, 9, 0)[:9].any()       # nothing is permuted: 0


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_the_longest_message_at_rate_one(ctx, field):
    """VDF_RO_HASH_MAX_LEN elements at width 2: 1,024 permutations, the longest run of the kernel"""
    check(ctx, NARROW, field, 1, MAX_LEN, 9, 250, (True,) * 4)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
@pytest.mark.parametrize("bits", BITS)
def test_truncations(ctx, field, bits):
    check(ctx, NEPTUNE, field, 2, 16, 9, bits)
    check(ctx, NARROW, field, 2, 3, 9, bits)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_tags(ctx, field):
    """two tags, and one above 2^32 whose sum with len << 32 carries out of bit 32"""
    for spec, ln in ((NEPTUNE, 7), (NARROW, 7)):
        for tag in (1, 2, (1 << 33) + 0xFFFFFFFF):
            check(ctx, spec, field, tag, ln, 9, 0)
        a = _hash(ctx, spec, field, 1, pool(field, ln, 9)[0], ln, 9, 0)
        b = _hash(ctx, spec, field, 2, pool(field, ln, 9)[0], ln, 9, 0)
        assert (a[:9] != b[:9]).any(axis=1).all()


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_one_non_zero_element_in_each_position(ctx, field):
    """a wrong lane assignment or a missing permutation after a short last block shows on these: width 9, up to two blocks and
    one element"""
    spec = spec_of(9, (8, 30))
    m = o.modulus(field)
    for ln in (1, 7, 8, 9, 17):
        msgs = [[0] * ln, [m - 1] * ln] + [[5 if k == j else 0 for k in range(ln)] for j in range(ln)]
        xs = mont([v for msg in msgs for v in msg], m).reshape(-1, 4)
        out = _hash(ctx, spec, field, 1, xs, ln, len(msgs), 0)
        want = np.zeros((len(msgs), 4), dtype="<u8")
        nova.ro_hash_batch_eval(field, 1, xs, ln, len(msgs), 0, want, ro=block(spec))
        assert np.array_equal(out[:len(msgs)], want), ln
        assert np.array_equal(out[:3], by_the_oracle(spec, field, 1, msgs[:3], 0)), ln
        assert len({bytes(r) for r in out[:len(msgs)]}) == len(msgs)


@pytest.mark.parametrize("field", FIELDS, ids=["Fp", "Fq"])
def test_host_and_device_pointers_in_each_position(ctx, field):
    for mask in range(16):
        check(ctx, NEPTUNE, field, 1, 13, 9, 250, tuple(bool(mask >> j & 1) for j in range(4)))


def test_two_runs_are_byte_equal(ctx):
    xs = pool(FIELD_FQ, 17, 1000)[0]
    a = _hash(ctx, NEPTUNE, FIELD_FQ, 1, xs, 17, 1000, 250, (True,) * 4)
    b = _hash(ctx, NEPTUNE, FIELD_FQ, 1, xs, 17, 1000, 250, (True,) * 4)
    assert a.tobytes() == b.tobytes()


def test_nothing_is_touched_for_no_messages(ctx):
    import torch
    rc, mds = consts(FIELD_FP, NEPTUNE)
    out = np.full((2, 4), FILL, dtype="<u8")
    ctx.ro_hash_batch_block(FIELD_FP, 1, 25, 8, 57, rc, mds, np.zeros((0, 4), dtype="<u8"), 3, 0, 250, out)
    ctx.ro_hash_batch_block(FIELD_FQ, 1, 25, 8, 57, None, None, None, 3, 0, 0, None)
    assert (out == FILL).all()
    dout = torch.from_numpy(out.view(np.int64).copy()).cuda()
    ctx.ro_hash_batch_block(FIELD_FP, 1, 25, 8, 57, dout, dout, dout, 3, 0, 128, dout)
    ctx.sync()
    assert (dout.cpu().numpy().view("<u8") == FILL).all()


def test_refusals(ctx):
    """each refusal is followed by one good call: the context goes on working"""
    import torch
    field, ln, n, spec = FIELD_FP, 3, 2, spec_of(9, (8, 30))
    t, rf, rp = spec.width, spec.full_rounds, spec.partial_rounds
    xs = np.array(pool(field, ln, 9)[0][:ln * n])
    want = reference(spec, field, 1, pool(field, ln, 9)[0], ln, 9, 250)[:n]
    out = np.full((n, 4), FILL, dtype="<u8")
    rc, mds = (np.array(x) for x in consts(field, spec))
    buf = torch.zeros(rc.nbytes + 64, dtype=torch.uint8, device="cuda")            # misaligned device pointers: 8 bytes off
    buf[8:8 + rc.nbytes] = torch.from_numpy(rc.view(np.uint8).reshape(-1).copy()).cuda()
    off = buf.data_ptr() + 8
    call = lambda field=field, t=t, rf=rf, rp=rp, rc=rc, mds=mds, xs=xs, ln=ln, bits=250, out=out: \
        ctx.ro_hash_batch_block(field, 1, t, rf, rp, rc, mds, xs, ln, n, bits, out)
    calls = {
        "a bad field": lambda: call(field=7),
        "width = 1": lambda: call(t=1),
        "width = 26": lambda: call(t=26),
        "full_rounds = 0": lambda: call(rf=0),
        "full_rounds = 7": lambda: call(rf=7),
        "full_rounds = 18": lambda: call(rf=18),
        "partial_rounds = -1": lambda: call(rp=-1),
        "partial_rounds = 129": lambda: call(rp=129),
        "bits = -1": lambda: call(bits=-1),
        "bits = 256": lambda: call(bits=256),
        "len = 1025": lambda: call(xs=np.zeros((1025 * n, 4), dtype="<u8"), ln=1025),
        "null rc": lambda: call(rc=None),
        "null mds": lambda: call(mds=None),
        "null xs": lambda: call(xs=None),
        "null out": lambda: call(out=None),
        "misaligned device rc": lambda: call(rc=off),
        "misaligned device mds": lambda: call(mds=off),
        "misaligned device xs": lambda: call(xs=off),
        "misaligned device out": lambda: call(out=off),
    }
    for name, refused in calls.items():
        with pytest.raises(VdfError) as e:
            refused()
        assert e.value.code == BAD_ARG, name
        assert (out == FILL).all(), name                                           # a refused call wrote nothing
        good = np.full((n, 4), FILL, dtype="<u8")
        call(out=good)
        assert np.array_equal(good, want), name
    call(xs=None, ln=0, bits=0)                                                    # xs may be null when len = 0
    assert not out.any()
