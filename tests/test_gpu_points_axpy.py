"""GPU: vdf_points_axpy (include/vdf_hip.h) -- out[i] = a[i] + s[i] b[i], one lane per entry, the per-entry folds of the
aggregate's device verifier.  The expected points are oracle/pasta.py's big-integer curve arithmetic alone, compared byte for
byte in canonical affine Montgomery form.  Every operand is a known multiple of the generator, so the expected point of an entry
is ((alpha + s' beta) mod order) G with s' = s mod 2^bits -- one fixed-base multiplication by pasta.pt_add over a table of
pasta.pt_add's own making; the first entries of every pool are checked against pasta.pt_mul(s', b) + a directly as well.

The call MASKS a scalar's bits at and above `bits` (the documented choice): the pools hold such scalars, and one test states it."""
import random

import numpy as np
import pytest

import vdf_amd
from oracle import pasta as o
from util import affine_array, limbs

pytestmark = pytest.mark.gpu
CURVES = [vdf_amd.CURVE_PALLAS, vdf_amd.CURVE_VESTA]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]               # wave and workgroup edges, and four workgroups
POOL = max(SIZES)
FILL = 0xA5A5A5A5A5A5A5A5
CLASSES = ("random", "a identity", "b identity", "both identity", "a = -s b", "a = s b", "a = b")
SCALARS = ("0", "1", "2", "2^128 - 1", "order - 1", "random")


class FixedBase:
    """k G by pasta.pt_add over the multiples d 256^j G"""
    def __init__(self, curve):
        self.m = o.curve_base_modulus(curve)
        self.order = o.curve_scalar_modulus(curve)
        self.rows = []
        base = o.generator(curve)
        for _ in range(32):
            row, acc = [None], None
            for _ in range(255):
                acc = o.pt_add(acc, base, self.m)
                row.append(acc)
            self.rows.append(row)
            base = o.pt_add(acc, base, self.m)

    def mul(self, k):
        k %= self.order
        acc = None
        for j in range(32):
            acc = o.pt_add(acc, self.rows[j][(k >> (8 * j)) & 0xFF], self.m)
        return acc


_FB, _B, _POOLS = {}, {}, {}


def fixed_base(curve):
    if curve not in _FB:
        _FB[curve] = FixedBase(curve)
    return _FB[curve]


def _scalar(kind, order, bits, rng):
    if kind == "0":
        return 0
    if kind == "1":
        return 1
    if kind == "2":
        return 2
    if kind == "2^128 - 1":
        return (1 << 128) - 1
    if kind == "order - 1":                                  # 255-bit runs only; a 128-bit run draws at random instead
        return order - 1 if bits == 255 else rng.getrandbits(128)
    pick = rng.randrange(4)
    if pick == 0:
        return rng.getrandbits(bits)                          # in range (a 255-bit one is at or above the order half the time)
    if pick == 1:
        return rng.getrandbits(256)                           # bits at and above `bits` set: masked
    if pick == 2:
        return rng.getrandbits(bits) | (1 << (bits - 1))      # the top counted bit set
    return rng.getrandbits(64)


def pool(curve, bits):
    """POOL entries of one curve and scalar length: (a, b uint64[n, 8]; s uint64[n, 4]; expected uint64[n, 8]; the entries' class
    and scalar kind), made once and never changed.  Entry i has class i mod 7 and scalar kind (i div 7) mod 6: the first 42
    entries hold every combination, so every size from 63 on has every class under every scalar."""
    key = (curve, bits)
    if key in _POOLS:
        return _POOLS[key]
    fb = fixed_base(curve)
    m, order = fb.m, fb.order
    if curve not in _B:                                       # b is the same for both scalar lengths
        rb = random.Random(0x61787079 + curve)
        betas = [rb.randrange(1, order) for _ in range(POOL)]
        _B[curve] = (betas, [fb.mul(k) for k in betas])
    betas, bpts = _B[curve]
    rng = random.Random(0x50A + 2 * bits + curve)
    a_pts, b_pts, scal, want, tags = [], [], [], [], []
    for i in range(POOL):
        cls, kind = CLASSES[i % 7], SCALARS[(i // 7) % 6]
        s = _scalar(kind, order, bits, rng)
        sm = s & ((1 << bits) - 1)
        beta, b = betas[i], bpts[i]
        alpha = rng.randrange(1, order)
        if cls in ("b identity", "both identity"):
            beta, b = 0, None
        if cls in ("a identity", "both identity"):
            alpha = 0
        elif cls == "a = -s b":
            alpha = -sm * beta % order
        elif cls == "a = s b":
            alpha = sm * beta % order
        elif cls == "a = b":
            alpha = beta
        a = fb.mul(alpha)
        a_pts.append(a); b_pts.append(b); scal.append(s); tags.append((cls, kind))
        want.append(fb.mul(alpha + sm * beta))
    for i in range(POOL):
        cls, kind = tags[i]
        if cls == "a = -s b":
            assert want[i] is None
        if cls == "a = b" and b_pts[i] is not None:
            assert a_pts[i] == b_pts[i]
    for i in range(14):                                       # the shortcut through the discrete logarithms, against the plain statement
        sm = scal[i] & ((1 << bits) - 1)
        assert want[i] == o.pt_add(a_pts[i], o.pt_mul(sm, b_pts[i], m), m), tags[i]
    out = (affine_array(a_pts, curve), affine_array(b_pts, curve), limbs(scal), affine_array(want, curve), tags)
    for arr in out[:4]:
        arr.setflags(write=False)
    _POOLS[key] = out
    return out


def _place(arr, on_device):
    if not on_device:
        return arr
    import torch
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()


def _axpy(ctx, curve, a, b, s, bits, placement=(False, False, False, False)):
    """out uint64[n, 8] of vdf_points_axpy, pre-filled so that an unwritten entry shows"""
    n = a.shape[0]
    out = np.full((n, 8), FILL, dtype="<u8")
    da, db, ds, dout = (_place(x.copy(), p) for x, p in zip((a, b, s, out), placement))
    ctx.points_axpy(curve, da, db, ds, bits, n, dout)
    ctx.sync()
    return dout if isinstance(dout, np.ndarray) else dout.cpu().numpy().view("<u8").reshape(n, 8)


@pytest.mark.parametrize("bits", [128, 255])
@pytest.mark.parametrize("curve", CURVES, ids=["pallas", "vesta"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_classes_and_memory_kinds(ctx, curve, bits, n):
    """every size from all-host arrays, all-device arrays and a mixture that changes with the size"""
    a, b, s, want, tags = pool(curve, bits)
    if n >= 63:
        assert {t for t in tags[:n]} == {(c, k) for c in CLASSES for k in SCALARS}
    k = SIZES.index(n)
    mixed = (bool(k & 1), bool(k & 2), bool(k & 4), not (k & 1))
    for placement in ((False,) * 4, (True,) * 4, mixed):
        out = _axpy(ctx, curve, a[:n], b[:n], s[:n], bits, placement)
        bad = np.nonzero((out != want[:n]).any(axis=1))[0]
        assert bad.size == 0, (placement, [(int(i), tags[i]) for i in bad[:8]])


@pytest.mark.parametrize("curve", CURVES, ids=["pallas", "vesta"])
def test_host_and_device_pointers_in_each_position(ctx, curve):
    a, b, s, want, _ = pool(curve, 128)
    n = 65
    for mask in range(16):
        placement = tuple(bool(mask >> j & 1) for j in range(4))
        assert np.array_equal(_axpy(ctx, curve, a[:n], b[:n], s[:n], 128, placement), want[:n]), placement


@pytest.mark.parametrize("bits", [128, 255])
def test_bits_at_and_above_the_length_are_masked(ctx, bits):
    curve = vdf_amd.CURVE_PALLAS
    a, b, s, want, _ = pool(curve, bits)
    n = 64
    lo = np.array(s[:n])
    hi = lo.copy()
    if bits == 128:
        lo[:, 2:] = 0
        hi[:, 2:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    else:
        lo[:, 3] &= np.uint64(0x7FFFFFFFFFFFFFFF)
        hi[:, 3] |= np.uint64(0x8000000000000000)
    out_lo, out_hi = _axpy(ctx, curve, a[:n], b[:n], lo, bits), _axpy(ctx, curve, a[:n], b[:n], hi, bits)
    assert np.array_equal(out_lo, want[:n]) and np.array_equal(out_hi, want[:n])


@pytest.mark.parametrize("curve", CURVES, ids=["pallas", "vesta"])
def test_two_runs_over_the_same_input_are_byte_equal(ctx, curve):
    a, b, s, want, _ = pool(curve, 255)
    first = _axpy(ctx, curve, a[:257], b[:257], s[:257], 255, (True,) * 4)
    second = _axpy(ctx, curve, a[:257], b[:257], s[:257], 255, (True,) * 4)
    assert first.tobytes() == second.tobytes() == want[:257].tobytes()


def test_nothing_is_touched_for_no_entries(ctx):
    import torch
    out = np.full((2, 8), FILL, dtype="<u8")
    empty = np.zeros((0, 8), dtype="<u8")
    ctx.points_axpy(vdf_amd.CURVE_VESTA, empty, empty, np.zeros((0, 4), dtype="<u8"), 255, 0, out)
    ctx.points_axpy(vdf_amd.CURVE_VESTA, None, None, None, 128, 0, None)
    assert (out == FILL).all()
    dout = torch.from_numpy(out.view(np.int64).copy()).cuda()
    ctx.points_axpy(vdf_amd.CURVE_PALLAS, dout, dout, dout, 128, 0, dout)
    ctx.sync()
    assert (dout.cpu().numpy().view("<u8") == FILL).all()


def test_refusals(ctx):
    a, b, s, want, _ = pool(vdf_amd.CURVE_PALLAS, 128)
    a, b, s = a[:2].copy(), b[:2].copy(), s[:2].copy()
    out = np.full((2, 8), FILL, dtype="<u8")
    for bits in (0, 1, 127, 129, 254, 256, -128):
        with pytest.raises(vdf_amd.VdfError) as e:
            ctx.points_axpy(vdf_amd.CURVE_PALLAS, a, b, s, bits, 2, out)
        assert e.value.code == 1
    with pytest.raises(vdf_amd.VdfError) as e:
        ctx.points_axpy(7, a, b, s, 128, 2, out)
    assert e.value.code == 1
    for hole in range(4):
        args = [a, b, s, out]
        args[hole] = None
        with pytest.raises(vdf_amd.VdfError) as e:
            ctx.points_axpy(vdf_amd.CURVE_PALLAS, args[0], args[1], args[2], 128, 2, args[3])
        assert e.value.code == 1
    assert (out == FILL).all()                                # a refused call wrote nothing
    ctx.points_axpy(vdf_amd.CURVE_PALLAS, a, b, s, 128, 2, out)   # and the context goes on working
    assert np.array_equal(out, want[:2])
