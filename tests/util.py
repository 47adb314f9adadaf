"""Shared helpers for the tests: data reshaping between Python ints and limb arrays, and the
affine normalisation used as the canonical form of a point."""
import numpy as np

from oracle import pasta as o


def limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).copy()


def ints(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


def mont(vals, m):
    return limbs([o.to_mont(v, m) for v in vals])


def unmont(arr, m):
    return [o.from_mont(v, m) for v in ints(arr)]


def jac_to_affine(jac_arr, curve):
    """uint64[12] Jacobian (Montgomery) -> canonical affine ints, identity = None."""
    m = o.curve_base_modulus(curve)
    X, Y, Z = unmont(np.asarray(jac_arr).reshape(3, 4), m)
    if Z == 0:
        return None
    zi = pow(Z, -1, m)
    return (X * zi * zi % m, Y * zi * zi * zi % m)


def affine_array(points, curve):
    """list of oracle points (None = identity) -> uint64[n, 8] Montgomery affine array."""
    m = o.curve_base_modulus(curve)
    flat = []
    for p in points:
        x, y = (0, 0) if p is None else p
        flat += [o.to_mont(x, m), o.to_mont(y, m)]
    return limbs(flat).reshape(-1, 8)


def rand_limbs(rng, n, top_mask=0x3FFFFFFFFFFFFFFF):
    """n uniformly random 254-bit values as uint64[n, 4] (always < p, q)."""
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(top_mask)
    return a


def hexes(lst):
    return [int(h, 16) for h in lst]


# ---- device buffers and MinRoot states (the GPU tests; torch and the libraries are imported where they are used) ------------

def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def host(tensor):
    return tensor.cpu().numpy().view("<u8")


def dev_read(ctx, ptr, nbytes):
    from vdf_amd._lib import lib
    out = np.zeros(nbytes // 8, dtype="<u8")
    assert lib.vdf_dev_memcpy(ctx.handle, out.ctypes.data, ptr, nbytes) == 0
    return out


def states_array(states):
    """[State] -> uint64[n, 12]"""
    return np.frombuffer(b"".join(s.x + s.y + s.i for s in states), dtype="<u8").reshape(-1, 12).copy()


def mont_states(rows, m):
    """[(x, y, i) ints] -> uint64[n, 12] Montgomery"""
    return np.frombuffer(b"".join(int(o.to_mont(v, m)).to_bytes(32, "little") for r in rows for v in r), dtype="<u8").reshape(-1, 12).copy()


def forward_segment_expected(cref, field, st, t):
    """What vdf_minroot_forward_segment must write for the chain that starts at `st` (uint64[3, 4], Montgomery), by the C
    restatement alone: (trace uint64[2 (t + 1), 4], i_end uint64[1, 4], words uint64[3t + 1, 4]) -- per round x_(j+1) from its
    evaluator's trace, its square and fourth power by ref_fe_mul twice, then the end counter."""
    L = cref.lib()
    so, tr = cref.fe_array(3), cref.fe_array(2 * (t + 1))
    L.ref_minroot_eval(field, 1, cref.p(st), t, cref.p(so), cref.p(tr))
    xs = np.ascontiguousarray(tr.reshape(t + 1, 2, 4)[1:, 0, :])
    sq, qd = cref.fe_array(t), cref.fe_array(t)
    L.ref_fe_mul(field, cref.p(xs), cref.p(xs), t, cref.p(sq))
    L.ref_fe_mul(field, cref.p(sq), cref.p(sq), t, cref.p(qd))
    return tr, so[2:3].copy(), np.concatenate([np.stack([xs, sq, qd], axis=1).reshape(3 * t, 4), so[2:3]])


def host_trace(vdf, s0, t):
    """(result, uint64[t + 1, 8]) of vdf_minroot_eval with its trace"""
    import ctypes as C
    from vdf_amd.minroot import State, _State, nova_lib
    buf = np.zeros((t + 1, 8), dtype="<u8")
    out = _State()
    assert nova_lib.vdf_minroot_eval(vdf.FIELD, int(vdf.eval_mode), C.byref(s0._c()), t, C.byref(out), buf.ctypes.data) == 0
    return State._from_c(out), buf
