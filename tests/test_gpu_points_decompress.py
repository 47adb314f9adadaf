"""GPU: vdf_fe_sqrt and vdf_points_decompress (include/vdf_hip.h) -- the wire's 32-byte point encoding decoded one lane per
point, by a Tonelli-Shanks root whose every trip count is fixed.  The expected values are the oracle's alone (oracle/pasta.py
sqrt_mod, oracle/wire.py decompress_point / compress_point), compared exactly, and the host decoder (nova.point_decompress) is
held to the same bytes.  A random element reaches 2-adic depth k with probability 2^(k - 32), so the depths are built: with
m - 1 = 2^32 T and 5 a generator of both multiplicative groups, a = 5^(2^(32-k) r) for odd r has a^T of order exactly 2^k."""
import random

import numpy as np
import pytest

import vdf_amd
from oracle import pasta as o, wire as w
from util import limbs, mont
from vdf_amd import nova

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 5003]            # wave and workgroup edges, and twenty workgroups
POOL = max(SIZES)
GARBAGE = 0xA5


def _field_mod(field):
    return o.P if field == vdf_amd.FIELD_FP else o.Q


def _even_root(a, m):
    y = o.sqrt_mod(a, m)
    if y is None:
        return None
    return y if y % 2 == 0 else m - y


def _place(arr, on_device):
    """the array as the call takes it: numpy (host) or a torch tensor on the GPU holding the same bytes"""
    if not on_device:
        return arr
    import torch
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()


def _back(buf, dtype, shape):
    if isinstance(buf, np.ndarray):
        return buf
    return buf.cpu().numpy().view(dtype).reshape(shape)


def _sqrt(ctx, field, a, placement=(False, False, False)):
    """(out uint64[n, 4], ok uint8[n]) of vdf_fe_sqrt, both pre-filled so that an unwritten entry shows"""
    n = a.shape[0]
    out = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype="<u8")
    ok = np.full(n, GARBAGE, dtype=np.uint8)
    da, dout, dok = _place(a, placement[0]), _place(out, placement[1]), _place(ok, placement[2])
    ctx.fe_sqrt(field, da, n, dout, dok)
    ctx.sync()
    return _back(dout, "<u8", (n, 4)), _back(dok, np.uint8, (n,))


def _decompress(ctx, curve, enc, placement=(False, False, False)):
    """(out uint64[n, 8], ok uint8[n]) of vdf_points_decompress over enc = uint8[n, 32], outputs pre-filled"""
    n = enc.shape[0]
    out = np.full((n, 8), 0xA5A5A5A5A5A5A5A5, dtype="<u8")
    ok = np.full(n, GARBAGE, dtype=np.uint8)
    denc, dout, dok = _place(enc, placement[0]), _place(out, placement[1]), _place(ok, placement[2])
    ctx.points_decompress(curve, denc, n, dout, dok)
    ctx.sync()
    return _back(dout, "<u8", (n, 8)), _back(dok, np.uint8, (n,))


def _expected(encs, curve):
    """the oracle's decoding of every 32-byte string: (uint64[n, 8] Montgomery, zero where refused; uint8[n])"""
    m = o.curve_base_modulus(curve)
    flat, ok = [], []
    for e in encs:
        try:
            pt = w.decompress_point(e, curve)
        except ValueError:
            flat += [0, 0]; ok.append(0)
            continue
        x, y = (0, 0) if pt is None else pt
        flat += [o.to_mont(x, m), o.to_mont(y, m)]
        ok.append(1)
    return limbs(flat).reshape(-1, 8), np.array(ok, dtype=np.uint8)


def _random_point(rng, m, parity):
    while True:
        x = rng.randrange(1, m)
        y = o.sqrt_mod((x * x * x + 5) % m, m)
        if y is not None:
            return (x, y if y % 2 == parity else m - y)


def _specials(m):
    """every rule of the encoding at its edge"""
    top = 1 << 255
    return [bytes(32),                                              # the identity
            top.to_bytes(32, "little"),                             # ... has one encoding: with the parity bit it is refused
            (m - 1).to_bytes(32, "little"),                         # x = -1: (-1, 2) lies on both curves
            ((m - 1) | top).to_bytes(32, "little"),
            m.to_bytes(32, "little"), (m | top).to_bytes(32, "little"),            # x = m: not canonical
            (m + 1).to_bytes(32, "little"), ((m + 1) | top).to_bytes(32, "little"),
            (top - 1).to_bytes(32, "little"), b"\xff" * 32]                          # all 255 low bits set
_CACHE = {}


def pool(curve):
    """POOL encodings of one curve, every kind mixed, and the oracle's decoding of them: made once per curve, never changed"""
    if curve not in _CACHE:
        m = o.curve_base_modulus(curve)
        rng = random.Random(0x77697265 + curve)
        encs = list(_specials(m))
        while len(encs) < POOL:
            kind = rng.randrange(5)
            if kind < 2:
                encs.append(w.compress_point(_random_point(rng, m, kind)))          # a point of either parity
            elif kind < 4:
                encs.append((rng.randrange(m) | (rng.randrange(2) << 255)).to_bytes(32, "little"))   # an x: half are on no point
            else:
                encs.append(rng.choice(_specials(m)))
        rng.shuffle(encs)
        arr = np.frombuffer(b"".join(encs), dtype=np.uint8).reshape(-1, 32).copy()
        arr.setflags(write=False)
        exp, ok = _expected(encs, curve)
        exp.setflags(write=False); ok.setflags(write=False)
        assert 0.2 < ok.mean() < 0.9                                                # both outcomes are well represented
        _CACHE[curve] = (encs, arr, exp, ok)
    return _CACHE[curve]


@pytest.mark.parametrize("field", [vdf_amd.FIELD_FP, vdf_amd.FIELD_FQ], ids=["fp", "fq"])
def test_the_root_at_every_2_adic_depth(ctx, field):
    m = _field_mod(field)
    T = (m - 1) >> 32
    assert T & 1 and pow(5, (m - 1) // 2, m) == m - 1 and pow(5, T << 31, m) == m - 1      # 5^T has order exactly 2^32
    vals, depth = [0, 1], [0, 0]
    for k in range(33):
        for r in (1, 3, 0x6D5A3F1):
            a = pow(5, (1 << (32 - k)) * r, m)
            aT = pow(a, T, m)
            assert pow(aT, 1 << k, m) == 1 and (k == 0 or pow(aT, 1 << (k - 1), m) != 1)
            vals.append(a); depth.append(k)
    roots = [_even_root(a, m) for a in vals]
    assert all((y is None) == (k == 32) for y, k in zip(roots, depth))
    want = mont([0 if y is None else y for y in roots], m)
    want_ok = np.array([0 if y is None else 1 for y in roots], dtype=np.uint8)
    a = mont(vals, m)
    for placement in ((False, False, False), (True, True, True)):
        out, ok = _sqrt(ctx, field, a, placement)
        assert np.array_equal(ok, want_ok)
        assert np.array_equal(out, want)


@pytest.mark.parametrize("field", [vdf_amd.FIELD_FP, vdf_amd.FIELD_FQ], ids=["fp", "fq"])
def test_the_root_of_random_elements_over_wave_edges(ctx, field):
    m = _field_mod(field)
    rng = random.Random(91 + field)
    vals = [rng.randrange(m) for _ in range(257)]
    roots = [_even_root(a, m) for a in vals]
    want = mont([0 if y is None else y for y in roots], m)
    want_ok = np.array([0 if y is None else 1 for y in roots], dtype=np.uint8)
    assert 64 < int(want_ok.sum()) < 192
    a = mont(vals, m)
    for n, placement in ((0, (False, False, False)), (1, (True, False, False)), (63, (False, True, False)), (64, (False, False, True)),
                         (65, (True, True, False)), (257, (False, True, True))):
        out, ok = _sqrt(ctx, field, a[:n].copy(), placement)
        assert np.array_equal(ok, want_ok[:n]) and np.array_equal(out, want[:n])


@pytest.mark.parametrize("curve", [vdf_amd.CURVE_PALLAS, vdf_amd.CURVE_VESTA], ids=["pallas", "vesta"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_memory_kinds(ctx, curve, n):
    """every size from all-host and from all-device arrays, and a mixture that changes with the size: each of the three arrays is
    tried from either kind of memory at every edge"""
    encs, arr, exp, exp_ok = pool(curve)
    k = SIZES.index(n)
    mixed = (bool(k & 1), bool(k & 2), not (k & 1))
    for placement in ((False, False, False), (True, True, True), mixed):
        out, ok = _decompress(ctx, curve, arr[:n].copy(), placement)
        assert ok.shape == (n,) and np.array_equal(ok, exp_ok[:n])
        assert np.array_equal(out, exp[:n])


def test_an_unaligned_slice_of_a_received_buffer(ctx):
    """the encodings sit at an odd address inside a larger device buffer: the kernel's byte path"""
    import torch
    curve = vdf_amd.CURVE_PALLAS
    encs, arr, exp, exp_ok = pool(curve)
    n = 70
    buf = torch.zeros(32 * n + 16, dtype=torch.uint8, device="cuda")
    for shift in (1, 4, 8):
        buf[shift:shift + 32 * n] = torch.from_numpy(arr[:n].reshape(-1).copy()).cuda()
        out = np.full((n, 8), 0xA5A5A5A5A5A5A5A5, dtype="<u8")
        ok = np.full(n, GARBAGE, dtype=np.uint8)
        ctx.points_decompress(curve, buf.data_ptr() + shift, n, out, ok)
        assert np.array_equal(ok, exp_ok[:n]) and np.array_equal(out, exp[:n])


@pytest.mark.parametrize("curve", [vdf_amd.CURVE_PALLAS, vdf_amd.CURVE_VESTA], ids=["pallas", "vesta"])
def test_every_kind_of_encoding_against_the_oracle_and_the_host_decoder(ctx, curve):
    m = o.curve_base_modulus(curve)
    rng = random.Random(5 + curve)
    groups = {
        "points of even y": [w.compress_point(_random_point(rng, m, 0)) for _ in range(12)],
        "points of odd y": [w.compress_point(_random_point(rng, m, 1)) for _ in range(12)],
        "specials": _specials(m),
        "random x": [(rng.randrange(m) | (rng.randrange(2) << 255)).to_bytes(32, "little") for _ in range(40)],
    }
    one_wave = groups["specials"] + groups["points of even y"][:10] + groups["points of odd y"][:10] + groups["random x"][:34]
    rng.shuffle(one_wave)
    assert len(one_wave) == 64
    groups["all of them in one wave"] = one_wave
    for name, encs in groups.items():
        arr = np.frombuffer(b"".join(encs), dtype=np.uint8).reshape(-1, 32).copy()
        exp, exp_ok = _expected(encs, curve)
        out, ok = _decompress(ctx, curve, arr)
        for i, e in enumerate(encs):
            assert ok[i] == exp_ok[i], (name, i, e.hex())
            assert np.array_equal(out[i], exp[i]), (name, i, e.hex())
            try:                                                    # the host decoder: the same verdict, the same bytes
                host = nova.point_decompress(e, curve)
            except vdf_amd.VdfError as ex:
                assert ex.code == 3 and ok[i] == 0, (name, i, e.hex())
            else:
                assert ok[i] == 1 and np.array_equal(host, out[i]), (name, i, e.hex())
    sp_ok = _expected(_specials(m), curve)[1]
    assert list(sp_ok) == [1, 0, 1, 1, 0, 0, 0, 0, 0, 0]
    assert 8 < int(_expected(groups["random x"], curve)[1].sum()) < 32              # about half the x values are on no point


@pytest.mark.parametrize("curve", [vdf_amd.CURVE_PALLAS, vdf_amd.CURVE_VESTA], ids=["pallas", "vesta"])
def test_round_trip(ctx, curve):
    m = o.curve_base_modulus(curve)
    rng = random.Random(17 + curve)
    pts = [None] + [_random_point(rng, m, i & 1) for i in range(99)]
    encs = [w.compress_point(p) for p in pts]
    arr = np.frombuffer(b"".join(encs), dtype=np.uint8).reshape(-1, 32).copy()
    out, ok = _decompress(ctx, curve, arr, (True, True, True))
    assert ok.all()
    assert [nova.point_compress(out[i], curve) for i in range(len(pts))] == encs


def test_bad_arguments(ctx):
    enc = np.zeros((1, 32), dtype=np.uint8)
    out, ok = np.zeros((1, 8), dtype="<u8"), np.zeros(1, dtype=np.uint8)
    with pytest.raises(vdf_amd.VdfError):
        ctx.points_decompress(7, enc, 1, out, ok)
    with pytest.raises(vdf_amd.VdfError):
        ctx.fe_sqrt(7, np.zeros((1, 4), dtype="<u8"), 1, np.zeros((1, 4), dtype="<u8"), ok)
    with pytest.raises(vdf_amd.VdfError):
        ctx.points_decompress(vdf_amd.CURVE_PALLAS, None, 1, out, ok)
