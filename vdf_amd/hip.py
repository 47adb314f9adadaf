"""Thin Python handle over the C ABI (include/vdf_hip.h).  Plumbing only: every arithmetic
operation is a HIP kernel behind `libvdf_hip.so`.  Buffers may be numpy arrays (host, staged by
the library over PCIe) or torch CUDA tensors (device, used in place)."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import lib, CURVE_PALLAS, CURVE_VESTA, FIELD_FP, FIELD_FQ  # noqa: F401


class HipTuning(C.Structure):
    """vdf_hip_tuning (include/vdf_hip.h): process-wide tuning of the kernels."""
    _fields_ = [("struct_size", C.c_uint32)] + [(k, C.c_int32) for k in (
        "msm_direct", "direct_priority", "direct_fused", "light_priority", "accumulate_fill", "accumulate_lds", "slice_len", "part_bits",
        "reduction", "reduction_quads", "heavy_min", "giant_span", "nifs_lanes", "shim_cache", "nifs_fused", "fold_u128", "fixup_serial", "sort_staged", "glv")]


def tuning_get() -> HipTuning:
    t = HipTuning()
    rc = lib.vdf_hip_tuning_get(C.byref(t))
    if rc != 0:
        raise VdfError(rc, "vdf_hip_tuning_get")
    return t


def tuning_set(**fields) -> HipTuning:
    """Changes the named fields of the process-wide tuning; returns the values now in force."""
    t = tuning_get()
    for k, v in fields.items():
        if k not in dict(HipTuning._fields_):
            raise KeyError(k)
        setattr(t, k, int(v))
    rc = lib.vdf_hip_tuning_set(C.byref(t))
    if rc != 0:
        raise VdfError(rc, "vdf_hip_tuning_set: a field is out of range")
    return t


class IpaOpening(C.Structure):
    """vdf_ipa_opening (include/vdf_hip.h): one opening of an inner-product argument for vdf_ipa_coefficients."""
    _fields_ = [("weight", C.c_uint64 * 4), ("k", C.c_int), ("log_m", C.c_int), ("lo", C.c_void_p), ("hi", C.c_void_p),
                ("pattern", C.c_void_p)]


class TapeOp(C.Structure):
    """vdf_tape_op: one op of a round tape (include/vdf_hip.h VDF_TAPE_*)."""
    _fields_ = [("op", C.c_uint8), ("dst", C.c_uint8), ("a", C.c_uint8), ("b", C.c_uint8)]


class RoundTapeC(C.Structure):
    _fields_ = [("ops", C.POINTER(TapeOp)), ("n_ops", C.c_size_t), ("consts", C.c_void_p), ("n_consts", C.c_size_t),
                ("n_slots", C.c_uint32), ("n_vars", C.c_uint32), ("n_cons", C.c_uint32), ("n_inv", C.c_uint32), ("n_adv", C.c_uint32),
                ("table", C.c_void_p), ("tab_rows", C.c_uint32), ("tab_cols", C.c_uint32)]


TAPE_MAX_OPS, TAPE_MAX_CONSTS, TAPE_MAX_SLOTS, TAPE_MAX_VARS, TAPE_MAX_INV, TAPE_MAX_ADV = 320, 24, 24, 64, 16, 8
WALK_MAX_SLOTS, WALK_MAX_WORK = 32, 1 << 23        # VDF_WALK_MAX_SLOTS, VDF_WALK_MAX_WORK
TAPE_MAX_LANES = 16                                # VDF_TAPE_MAX_LANES
FORWARD_TAPE_MAX_WORK = 1 << 20                    # VDF_FORWARD_TAPE_MAX_WORK
TAPE_POW = 9                                       # VDF_TAPE_POW
TAPE_POWC = 10                                     # VDF_TAPE_POWC
TAPE_TAB = 11                                      # VDF_TAPE_TAB
TAPE_MAX_TAB_ROWS, TAPE_MAX_TAB_COLS = 4096, 8     # VDF_TAPE_MAX_TAB_ROWS, VDF_TAPE_MAX_TAB_COLS


class RoundTape:
    """vdf_round_tape with the arrays it points into (vdf_amd.nova.record_round_body makes one).  table: the numpy array
    uint64[rows, cols, 4] of a tape that holds a TAPE_TAB (None without one); `c` names it as HOST memory, which is what the host
    evaluators of vdf_amd.nova read, and the Context.round_tape_* methods hand the kernels a device copy in its place."""

    def __init__(self):
        self.ops = (TapeOp * TAPE_MAX_OPS)()
        self.consts = np.zeros((TAPE_MAX_CONSTS, 4), dtype="<u8")
        self.c = RoundTapeC()
        self.table = None

    def set_table(self, table) -> None:
        """Gives the tape the table uint64[rows, cols, 4] (Montgomery form), or none (None)."""
        if table is None:
            self.table, self.c.table, self.c.tab_rows, self.c.tab_cols = None, None, 0, 0
            return
        table = np.ascontiguousarray(table, dtype="<u8")
        if table.ndim != 3 or table.shape[2] != 4:
            raise ValueError("a tape's table is uint64[rows, cols, 4]")
        self.table = table
        self.c.table, self.c.tab_rows, self.c.tab_cols = table.ctypes.data, table.shape[0], table.shape[1]

    def op_list(self):
        return [(o.op, o.dst, o.a, o.b) for o in self.ops[:self.c.n_ops]]


TERM_SEG, TERM_ABS, TERM_NO_SLOPE = 0, 1, 0xFF      # VDF_TERM_*
PERIODIC_MAX_ROW_TERMS, PERIODIC_MAX_ROWS, PERIODIC_MAX_TERMS, PERIODIC_MAX_CONSTS = 8, 32, 128, 24      # VDF_PERIODIC_MAX_*


class PeriodicTerm(C.Structure):
    """vdf_periodic_term: one term of a periodic row (include/vdf_hip.h VDF_TERM_*); col is a signed offset under TERM_SEG."""
    _fields_ = [("kind", C.c_uint8), ("c0", C.c_uint8), ("c1", C.c_uint8), ("pad", C.c_uint8), ("col", C.c_uint32)]


class PeriodicRowsC(C.Structure):
    _fields_ = [("n_cons", C.c_uint32), ("n_vars", C.c_uint32), ("j0", C.c_uint64), ("row_start", C.c_void_p),
                ("terms", C.POINTER(PeriodicTerm)), ("n_terms", C.c_size_t), ("consts", C.c_void_p), ("n_consts", C.c_size_t)]


class PeriodicRows:
    """vdf_periodic_rows with the arrays it points into (vdf_amd.nova.periodic_rows_detect / shape_periodic_custom make one).
    lead, row_begin, row_count: the repetitions and rows the detection found it for (0 when made by hand)."""

    def __init__(self):
        self.row_start = np.zeros(3 * PERIODIC_MAX_ROWS + 1, dtype=np.uint16)
        self.terms = (PeriodicTerm * PERIODIC_MAX_TERMS)()
        self.consts = np.zeros((PERIODIC_MAX_CONSTS, 4), dtype="<u8")
        self.c = PeriodicRowsC()
        self.c.row_start = self.row_start.ctypes.data
        self.c.terms = C.cast(self.terms, C.POINTER(PeriodicTerm))
        self.c.consts = self.consts.ctypes.data
        self.lead = self.row_begin = self.row_count = 0

    def term_list(self):
        """[[(kind, signed col, c0, c1) per term] per matrix A, B, C] per row"""
        rel = lambda t: t.col - (1 << 32) if t.kind == TERM_SEG and t.col >= 1 << 31 else t.col
        rs = self.row_start
        return [[[(t.kind, rel(t), t.c0, t.c1) for t in self.terms[rs[3 * c + k]:rs[3 * c + k + 1]]] for k in range(3)]
                for c in range(self.c.n_cons)]


class VdfError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vdf_hip error {code}: {msg}")
        self.code = code


def ints_to_limbs(vals: Sequence[int]) -> np.ndarray:
    """Python ints -> uint64[n, 4] little-endian limbs (data reshaping, no arithmetic)."""
    buf = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).copy()


def limbs_to_ints(arr: np.ndarray) -> list:
    a = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, 4)
    raw = a.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(a.shape[0])]


def _ptr(x) -> Optional[int]:
    """Address of a numpy array or torch tensor (None stays None)."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("numpy buffers must be C-contiguous")
        return x.ctypes.data
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("tensors must be contiguous")
        return x.data_ptr()
    if isinstance(x, int):
        return x
    raise TypeError(type(x))


class Bases:
    def __init__(self, ctx: "Context", handle: int, curve: int):
        self.ctx, self.handle, self.curve = ctx, handle, curve
        ctx._children.add(self)

    def __len__(self) -> int:
        return lib.vdf_bases_len(self.handle)

    def validate(self) -> None:
        """Raises VdfError (NONCANONICAL / BAD_ARG, with the first offending index) unless every point is valid."""
        bad = C.c_size_t()
        rc = lib.vdf_bases_validate(self.ctx.handle, self.handle, C.byref(bad))
        if rc != 0:
            raise VdfError(rc, (lib.vdf_last_error(self.ctx.handle) or b"").decode() + f" (index {bad.value})")

    @property
    def device_ptr(self) -> int:
        return lib.vdf_bases_device_ptr(self.handle)

    def precompute(self, window_bits: int = 16, sets: int = 1) -> None:
        self.ctx._check(lib.vdf_bases_precompute(self.ctx.handle, self.handle, window_bits, sets))

    @property
    def window(self) -> int:
        """Window of the fixed-base table (0 without one)."""
        return lib.vdf_bases_window(self.handle)

    def precompute_digits(self, ranges, window_bits: int = 0) -> None:
        """Digit table over the generator ranges [(begin, count), ...] (at most 4): MSMs inside them of up to 2^17 scalars
        become a plain sum of gathered multiples (vdf_hip.h vdf_bases_precompute_digits).  [] drops the table."""
        k = len(ranges)
        b = (C.c_size_t * max(k, 1))(*[int(r[0]) for r in ranges])
        n = (C.c_size_t * max(k, 1))(*[int(r[1]) for r in ranges])
        self.ctx._check(lib.vdf_bases_precompute_digits(self.ctx.handle, self.handle, window_bits, k, b, n))

    @property
    def digit_window(self) -> int:
        return lib.vdf_bases_digit_window(self.handle)

    def download(self, offset: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = len(self) - offset if n is None else n
        out = np.zeros((n, 8), dtype="<u8")
        self.ctx._check(lib.vdf_bases_download(self.ctx.handle, self.handle, offset, n, _ptr(out)))
        return out

    def free(self) -> None:
        # if the context is already gone (finalisers run in no particular order at interpreter shutdown) the
        # device memory went with it: calling into the library with a dead context would be a use after free
        if self.handle and self.ctx.handle:
            lib.vdf_bases_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)     # vdf_allgather_fn


def msm_multi(ctxs, bases, scalars, n, offsets=None, is_mont: bool = False):
    """vdf_msm_multi: one process, one Context / generator shard / scalar slice per device; returns uint64[12]."""
    k = len(ctxs)
    out = np.zeros(12, dtype="<u8")
    offs = (C.c_size_t * k)(*(offsets or [0] * k))
    rc = lib.vdf_msm_multi((C.c_void_p * k)(*[c.handle for c in ctxs]), (C.c_void_p * k)(*[b.handle for b in bases]), offs,
                           (C.c_void_p * k)(*[_ptr(x) for x in scalars]), (C.c_size_t * k)(*[int(x) for x in n]), k,
                           int(is_mont), out.ctypes.data)
    ctxs[0]._check(rc)
    return out


class Shape:
    def __init__(self, ctx: "Context", handle: int, field: int, num_cons: int, num_cols: int):
        self.ctx, self.handle, self.field, self.num_cons, self.num_cols = ctx, handle, field, num_cons, num_cols
        ctx._children.add(self)

    def free(self) -> None:
        if self.handle and self.ctx.handle:      # see Bases.free
            lib.vdf_shape_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MsmJob:
    """Handle of an open MSM job; finish() ends it in every case."""

    def __init__(self, ctx: "Context", handle: int, k: int):
        self.ctx, self.handle, self.k = ctx, handle, k

    def push(self, g: int, scalars) -> None:
        self.ctx._check(lib.vdf_msm_job_push(self.handle, g, _ptr(scalars)))

    def finish(self, out=None):
        if out is None:
            out = np.zeros((self.k, 12), dtype="<u8")
        h, self.handle = self.handle, None
        self.ctx._check(lib.vdf_msm_job_finish(h, _ptr(out)))
        return out


QUEUE_CRITICAL, QUEUE_SIDE = 1, 2


class _TapeTable:
    """One context's device copy of one tape's table (Context._tape): the array it was made from (identity decides whether the
    copy still is the tape's table), its size, and the vdf_round_tape handed to the launchers in the tape's place."""

    def __init__(self, tape, array, d_table, nbytes):
        self.tape, self.array, self.d_table, self.nbytes = weakref.ref(tape), array, d_table, nbytes
        self.c = RoundTapeC()
        self.finalizer = None


class Context:
    """One context per GPU (one process per GPU)."""

    def __init__(self, device: int = 0, pooled_role: int = 0):
        """pooled_role: 0 = a context with a stream of its own (vdf_ctx_create); QUEUE_CRITICAL / QUEUE_SIDE = a stream from the
        device's pool of hardware queues, shared once the budget is spent (vdf_ctx_create_pooled)."""
        h = C.c_void_p()
        dev = C.c_int(device)
        rc = (lib.vdf_ctx_create_pooled(C.byref(dev), 1, pooled_role, C.byref(h)) if pooled_role
              else lib.vdf_ctx_create(C.byref(dev), 1, C.byref(h)))
        if rc != _lib.VDF_OK:
            raise VdfError(rc, (lib.vdf_last_error(None) or b"").decode())
        self.handle = h.value
        self.device = device
        self._children = weakref.WeakSet()      # handles that own device memory of this context
        self._tape_tables = {}                  # id(tape) -> _TapeTable: the device copy of a live tape's table (_tape)

    def _check(self, rc: int) -> None:
        if rc != _lib.VDF_OK:
            raise VdfError(rc, (lib.vdf_last_error(self.handle) or b"").decode())

    def __enter__(self) -> "Context":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def close(self) -> None:
        if self.handle:
            for child in list(self._children):   # bases / shapes must go before their context
                child.free()
            for ent in self._tape_tables.values():
                ent.finalizer.detach()
                lib.vdf_dev_free(self.handle, ent.d_table)
            self._tape_tables = {}
            lib.vdf_ctx_destroy(self.handle)
            self.handle = None

    def queue_info(self) -> dict:
        """{"pooled", "sharers", "device_streams"}: vdf_ctx_queue_info."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(lib.vdf_ctx_queue_info(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"pooled": bool(a.value), "sharers": b.value, "device_streams": c.value}

    def set_stream(self, stream_ptr) -> None:
        """A foreign hipStream_t (e.g. a torch stream's .cuda_stream); None / 0 = back to the context's own."""
        self._check(lib.vdf_ctx_set_stream(self.handle, stream_ptr or None))

    @property
    def stream(self) -> int:
        return lib.vdf_ctx_get_stream(self.handle)

    def set_async(self, flag: bool) -> None:
        self._check(lib.vdf_ctx_set_async(self.handle, int(flag)))

    def get_async(self) -> bool:
        v = C.c_int()
        self._check(lib.vdf_ctx_get_async(self.handle, C.byref(v)))
        return bool(v.value)

    def sync(self) -> None:
        self._check(lib.vdf_ctx_sync(self.handle))

    def wait(self, other: "Context") -> None:
        """Work enqueued on this context from now on starts after everything enqueued on `other` so far."""
        self._check(lib.vdf_ctx_wait(self.handle, other.handle))

    def mark(self, slot: int = 0) -> None:
        """Remembers the current end of this context's queue under `slot` (0..3)."""
        self._check(lib.vdf_ctx_mark(self.handle, slot))

    def sync_mark(self, slot: int = 0) -> None:
        """Waits for everything enqueued before mark `slot`; later work keeps running."""
        self._check(lib.vdf_ctx_sync_mark(self.handle, slot))

    def wait_mark(self, other: "Context", slot: int = 0) -> None:
        """Work enqueued on this context from now on starts after `other` has reached its mark `slot` (not after what
        `other` was given since)."""
        self._check(lib.vdf_ctx_wait_mark(self.handle, other.handle, slot))

    def set_accumulate_fill(self, workgroups_per_cu: int) -> None:
        """Resident accumulation workgroups per CU this context's bucket-method MSMs fill (1..3; 0 = the process-wide value)."""
        self._check(lib.vdf_ctx_set_accumulate_fill(self.handle, workgroups_per_cu))

    def set_msm_window(self, c: int) -> None:
        self._check(lib.vdf_ctx_set_msm_window(self.handle, c))

    # ---- bases -------------------------------------------------------------------------
    def bases_upload(self, curve: int, pts) -> Bases:
        n = pts.shape[0]
        h = C.c_void_p()
        self._check(lib.vdf_bases_upload(self.handle, curve, _ptr(pts), n, C.byref(h)))
        return Bases(self, h.value, curve)

    def bases_generate(self, curve: int, seed: int, n: int, start: int = 0, family: int = 0) -> Bases:
        """family 0: P_i = [k_i]G (known discrete logs); 1: try-and-increment (unknown discrete logs)."""
        h = C.c_void_p()
        self._check(lib.vdf_bases_generate_family(self.handle, curve, family, seed, start, n, C.byref(h)))
        return Bases(self, h.value, curve)

    def bases_generate_label(self, curve: int, label: bytes, n: int, start: int = 0) -> Bases:
        """Generators derived from a label (SHAKE256 -> curve points): include/vdf_hip.h vdf_bases_generate_label."""
        h = C.c_void_p()
        buf = (C.c_uint8 * max(len(label), 1)).from_buffer_copy(label or b"\0")
        self._check(lib.vdf_bases_generate_label(self.handle, curve, buf, len(label), start, n, C.byref(h)))
        return Bases(self, h.value, curve)

    # ---- msm ---------------------------------------------------------------------------
    def msm(self, bases: Bases, scalars, n: Optional[int] = None, offset: int = 0, is_mont: bool = False, out=None):
        """Returns the Jacobian result as uint64[12] (numpy) unless `out` (device tensor) is given."""
        n = scalars.shape[0] if n is None else n
        host_out = out is None
        if host_out:
            out = np.zeros(12, dtype="<u8")
        self._check(lib.vdf_msm(self.handle, bases.handle, offset, _ptr(scalars), n, int(is_mont), _ptr(out)))
        return out

    def msm_batch(self, bases: Bases, scalars, n=None, offsets=None, is_mont: bool = False, out=None):
        """k <= 4 MSMs over the same generators in one pipeline; returns uint64[k, 12] unless `out` is given."""
        k = len(scalars)
        n = [s.shape[0] for s in scalars] if n is None else list(n)
        offsets = [0] * k if offsets is None else list(offsets)
        if out is None:
            out = np.zeros((k, 12), dtype="<u8")
        sc = (C.c_void_p * k)(*[_ptr(x) for x in scalars])
        self._check(lib.vdf_msm_batch(self.handle, bases.handle, k, (C.c_size_t * k)(*offsets), sc, (C.c_size_t * k)(*n),
                                      int(is_mont), _ptr(out)))
        return out

    def msm_job(self, bases: Bases, n, offsets=None, is_mont: bool = False) -> "MsmJob":
        """Start an MSM job over k = len(n) vectors (see include/vdf_hip.h): push them one at a time, then finish."""
        k = len(n)
        offsets = [0] * k if offsets is None else list(offsets)
        h = C.c_void_p()
        self._check(lib.vdf_msm_job_begin(self.handle, bases.handle, k, (C.c_size_t * k)(*offsets), (C.c_size_t * k)(*n),
                                          int(is_mont), C.byref(h)))
        return MsmJob(self, h.value, k)

    def msm_sharded(self, bases: Bases, scalars, n: int, rank: int, world: int, all_gather, partial, gathered, out,
                    is_mont: bool = False, always_gather: bool = False, offset: int = 0):
        """vdf_msm_sharded: this rank's partial, the host's all-gather of the world partials, the local point sum.
        all_gather(dst, src) is the collective on the caller's buffers `gathered` (world x 12 words) and `partial` (12),
        both device memory; it is called once, from inside the library, ordered after the partial.  The header's contract
        is that the collective runs ON the stream the library hands over (the one the partial was produced on and the
        point sum will run on): when the buffers are torch tensors the callback therefore makes that stream torch's
        current one for the duration of the call, whatever stream the caller happens to be on."""
        err = []

        def cb(_user, _send, _recv, _bytes, _stream):
            try:
                if hasattr(partial, "data_ptr"):
                    import torch
                    with torch.cuda.stream(torch.cuda.ExternalStream(int(_stream or 0), device=partial.device)):
                        all_gather(gathered, partial)
                else:
                    all_gather(gathered, partial)
                return 0
            except Exception as e:            # an exception must not unwind through the C frames
                err.append(e)
                return 1
        fn = _ALLGATHER(cb)
        rc = lib.vdf_msm_sharded(self.handle, bases.handle, offset, _ptr(scalars), n, int(is_mont), rank, world, fn, None,
                                 1 if always_gather else 0, _ptr(partial), _ptr(gathered), _ptr(out))
        if err:
            raise err[0]
        self._check(rc)
        return out

    def point_sum(self, curve: int, points, n: int, out=None):
        host_out = out is None
        if host_out:
            out = np.zeros(12, dtype="<u8")
        self._check(lib.vdf_point_sum(self.handle, curve, _ptr(points), n, _ptr(out)))
        return out

    def set_timing(self, flag: bool) -> None:
        self._check(lib.vdf_ctx_set_timing(self.handle, int(flag)))

    def msm_timing(self):
        """(sort_ms, accumulate_ms, tail_ms, total_ms, calls) summed since the last query."""
        ms = (C.c_float * 4)()
        calls = C.c_int()
        self._check(lib.vdf_msm_timing(self.handle, ms, C.byref(calls)))
        return (*[float(x) for x in ms], calls.value)

    # ---- shape / spmv --------------------------------------------------------------------
    def shape_create(self, field: int, num_cons: int, num_cols: int, mats) -> Shape:
        """mats: three (rows uint32[nnz], cols uint32[nnz], vals uint64[nnz,4]) triples (host)."""
        rows = (C.c_void_p * 3)(*[_ptr(m[0]) for m in mats])
        cols = (C.c_void_p * 3)(*[_ptr(m[1]) for m in mats])
        vals = (C.c_void_p * 3)(*[_ptr(m[2]) for m in mats])
        nnz = (C.c_size_t * 3)(*[int(m[0].shape[0]) for m in mats])
        h = C.c_void_p()
        self._check(lib.vdf_shape_create(self.handle, field, num_cons, num_cols, rows, cols, vals, nnz, C.byref(h)))
        self._keep = mats
        return Shape(self, h.value, field, num_cons, num_cols)

    def spmv3(self, shape: Shape, z, az, bz, cz) -> None:
        self._check(lib.vdf_spmv3(self.handle, shape.handle, _ptr(z), _ptr(az), _ptr(bz), _ptr(cz)))

    # ---- vector ops ------------------------------------------------------------------------
    def cross_term(self, field, az1, bz1, cz1, az2, bz2, cz2, u1, n, out) -> None:
        self._check(lib.vdf_cross_term(self.handle, field, _ptr(az1), _ptr(bz1), _ptr(cz1), _ptr(az2), _ptr(bz2),
                                       _ptr(cz2), _ptr(u1), n, _ptr(out)))

    def axpy(self, field, a, r, b, n, out) -> None:
        self._check(lib.vdf_axpy(self.handle, field, _ptr(a), _ptr(r), _ptr(b), n, _ptr(out)))

    # ---- folding two relaxed instances: u1, u2, r are HOST arrays, every vector is device memory ----
    def cross_term_relaxed(self, field, az1, bz1, cz1, u1, az2, bz2, cz2, u2, n, out) -> None:
        """T = Az1 o Bz2 + Az2 o Bz1 - u1 Cz2 - u2 Cz1 (vdf_hip.h vdf_cross_term_relaxed)."""
        self._check(lib.vdf_cross_term_relaxed(self.handle, field, _ptr(az1), _ptr(bz1), _ptr(cz1), _ptr(u1), _ptr(az2), _ptr(bz2),
                                               _ptr(cz2), _ptr(u2), n, _ptr(out)))

    def fold_relaxed(self, field, r, n, az1, bz1, cz1, e1, az2, bz2, cz2, e2, T) -> None:
        """In place: Az1 += r Az2, Bz1 += r Bz2, Cz1 += r Cz2, E1 += r T + r^2 E2 (vdf_hip.h vdf_fold_relaxed)."""
        self._check(lib.vdf_fold_relaxed(self.handle, field, _ptr(r), n, _ptr(az1), _ptr(bz1), _ptr(cz1), _ptr(e1), _ptr(az2), _ptr(bz2),
                                         _ptr(cz2), _ptr(e2), _ptr(T)))

    def minroot_witness(self, field, trace_xy, i0, t, out) -> None:
        self._check(lib.vdf_minroot_witness(self.handle, field, _ptr(trace_xy), _ptr(i0), t, _ptr(out)))

    # ---- fused step operations: scalar operands are HOST arrays, vectors are device buffers ----
    def minroot_step_z(self, field, trace_xy, t, z_in, i0, u, X, z) -> None:
        self._check(lib.vdf_minroot_step_z(self.handle, field, _ptr(trace_xy), t, _ptr(z_in), _ptr(i0), _ptr(u), _ptr(X),
                                           _ptr(z)))

    def minroot_step_z_packed(self, field, trace_xy, t, z_in, i0, u, X, z, w_packed) -> None:
        self._check(lib.vdf_minroot_step_z_packed(self.handle, field, _ptr(trace_xy), t, _ptr(z_in), _ptr(i0), _ptr(u),
                                                  _ptr(X), _ptr(z), _ptr(w_packed)))

    def minroot_step_segment(self, field, trace_xy, t, i0, vars_per_round, out) -> None:
        self._check(lib.vdf_minroot_step_segment(self.handle, field, _ptr(trace_xy), t, _ptr(i0), vars_per_round, _ptr(out)))

    def minroot_forward_segment(self, field, trace_xy, t, i_end, out) -> None:
        """The forward step circuit's 3t + 1 variables: x_(j+1), its square and fourth power per round, then final_i = i_end."""
        self._check(lib.vdf_minroot_forward_segment(self.handle, field, _ptr(trace_xy), t, _ptr(i_end), _ptr(out)))

    def minroot_forward_segment_lanes(self, field, trace_xy, lane_stride, t, lanes, i_end, out) -> None:
        """The same for `lanes` traces lane_stride entries apart, lane-major into out, in one launch; i_end: `lanes` host elements."""
        self._check(lib.vdf_minroot_forward_segment_lanes(self.handle, field, _ptr(trace_xy), lane_stride, t, lanes, _ptr(i_end), _ptr(out)))

    def _tape(self, tape: "RoundTape") -> int:
        """Address of the vdf_round_tape a launcher takes: the tape's own, or for a tape with a table a copy of it whose `table`
        is this context's device copy of that table.  The copy is made once per (tape, table array) -- the array's contents as
        they were then -- and made again when the tape has been given another array (RoundTape.set_table, or a new `table`); it
        is freed when the tape is collected or the context closed.  The dimensions a kernel is handed never exceed the copy."""
        if tape.table is None:
            return C.addressof(tape.c)
        ent = self._tape_tables.get(id(tape))
        if ent is not None and (ent.tape() is not tape or ent.array is not tape.table):
            self._drop_tape_table(id(tape), ent)      # another table: the old copy goes, a kernel never sees it under the new dimensions
            ent = None
        if ent is None:
            array = tape.table
            p = C.c_void_p()
            self._check(lib.vdf_dev_alloc(self.handle, array.nbytes, C.byref(p)))
            rc = lib.vdf_dev_memcpy(self.handle, p.value, array.ctypes.data, array.nbytes)
            if rc == _lib.VDF_OK:
                rc = lib.vdf_ctx_sync(self.handle)
            if rc != _lib.VDF_OK:
                lib.vdf_dev_free(self.handle, p.value)
                self._check(rc)
            ent = _TapeTable(tape, array, p.value, array.nbytes)
            ent.finalizer = weakref.finalize(tape, Context._tape_collected, weakref.ref(self), id(tape), ent)
            self._tape_tables[id(tape)] = ent
        if tape.c.tab_rows * tape.c.tab_cols * 32 > ent.nbytes:      # (a kernel would read past the device copy)
            raise ValueError("tab_rows x tab_cols exceeds the tape's table")
        c = ent.c
        for name, _ in RoundTapeC._fields_:      # (ops and counts as they are now: a test may patch a tape between two calls)
            setattr(c, name, getattr(tape.c, name))
        c.table = ent.d_table
        return C.addressof(c)

    def _drop_tape_table(self, key, ent) -> None:
        if self._tape_tables.get(key) is ent:
            del self._tape_tables[key]
            ent.finalizer.detach()
            if self.handle:
                lib.vdf_dev_free(self.handle, ent.d_table)

    @staticmethod
    def _tape_collected(ctx_ref, key, ent) -> None:
        ctx = ctx_ref()
        if ctx is not None:                      # (a closed context has freed every copy already)
            ctx._drop_tape_table(key, ent)

    def round_tape_run(self, field, tape: "RoundTape", t, inv, advice, out) -> None:
        """t repetitions of a recorded round, one GPU thread each: out (device, t * n_vars elements); inv: host, advice: device."""
        self._check(lib.vdf_round_tape_run(self.handle, field, self._tape(tape), t, _ptr(inv), _ptr(advice), _ptr(out)))

    def round_tape_walk(self, field, tape: "RoundTape", inv, entries, n, rounds, trace=None, walk_stride=0, top=0, group=0, group_stride=0,
                        j_base=0, j_group_step=0, heads=False, expect=None, ok=None) -> None:
        """n walks of `rounds` rounds of a recorded walk body in place over `entries` (device, n x n_adv elements), one lane each;
        strides in entries.  trace (device or None): walk w writes the entry it stands on before round r to entry
        (w // group) * group_stride + (w % group) * walk_stride + top - r; heads: a group's first walk also writes its landing.
        expect / ok (device, int32[n]): ok[w] = the landing equals expect[w].  inv: host."""
        self._check(lib.vdf_round_tape_walk(self.handle, field, self._tape(tape), _ptr(inv), _ptr(entries), n, rounds, _ptr(trace),
                                            walk_stride, top, group, group_stride, j_base, j_group_step, int(bool(heads)), _ptr(expect),
                                            _ptr(ok)))

    def round_tape_run_lanes(self, field, tape: "RoundTape", t, lanes, inv, advice, lane_stride, out) -> None:
        """round_tape_run for `lanes` advice arrays lane_stride entries apart in ONE launch: lane l's t * n_vars variables at
        out + l * t * n_vars, under its own inv[l * n_inv:(l + 1) * n_inv] (host, lanes * n_inv elements); advice, out: device."""
        self._check(lib.vdf_round_tape_run_lanes(self.handle, field, self._tape(tape), t, lanes, _ptr(inv), _ptr(advice), lane_stride,
                                                 _ptr(out)))

    def round_tape_walk_lanes(self, field, tape: "RoundTape", lanes, inv, entries, n, rounds, trace=None, walk_stride=0, top=0, group=0,
                              group_stride=0, j_base=None, j_group_step=0, heads=False, expect=None, ok=None) -> None:
        """round_tape_walk with the groups numbered step-major, lane-minor, in ONE launch: group G = w // group is lane G % lanes of
        step G // lanes, its trace at G * group_stride; its rounds see j_base[lane] + (G // lanes) * j_group_step + k - 1 and
        inv[lane * n_inv:(lane + 1) * n_inv].  inv (lanes * n_inv elements) and j_base (`lanes` ints, default zeros): host."""
        jb = np.ascontiguousarray([0] * lanes if j_base is None else [int(v) % 2**64 for v in j_base], dtype="<u8")
        if jb.size < lanes:
            raise ValueError("j_base: one counter per lane")
        self._check(lib.vdf_round_tape_walk_lanes(self.handle, field, self._tape(tape), lanes, _ptr(inv), _ptr(entries), n, rounds,
                                                  _ptr(trace), walk_stride, top, group, group_stride, jb.ctypes.data, j_group_step,
                                                  int(bool(heads)), _ptr(expect), _ptr(ok)))

    def round_tape_rebuild_lanes(self, field, forward_tape: "RoundTape", lanes, inv, entries, n, rounds, trace=None, walk_stride=0, base=0,
                                 group=0, group_stride=0, j_base=None, j_group_step=0, heads=False, expect=None, ok=None) -> None:
        """round_tape_walk_lanes ascending, by a FORWARD tape (POW, POWC and TAB admitted): walk w of group G = w // group (lane
        G % lanes of step G // lanes) has `base` rounds behind it, stands on local index k = (w % group) * walk_stride + base + r
        before round r, sees j_base[lane] + (G // lanes) * j_group_step + k there and writes what it produces to trace entry
        G * group_stride + k + 1; heads: a group's first walk also writes the entry it starts on.  expect / ok (device, int32[n]):
        ok[w] = where the walk stands afterwards equals expect[w].  inv (lanes * n_inv elements), j_base (`lanes` ints): host."""
        jb = np.ascontiguousarray([0] * lanes if j_base is None else [int(v) % 2**64 for v in j_base], dtype="<u8")
        if jb.size < lanes:
            raise ValueError("j_base: one counter per lane")
        self._check(lib.vdf_round_tape_rebuild_lanes(self.handle, field, self._tape(forward_tape), lanes, _ptr(inv), _ptr(entries), n, rounds,
                                                     _ptr(trace), walk_stride, base, group, group_stride, jb.ctypes.data, j_group_step,
                                                     int(bool(heads)), _ptr(expect), _ptr(ok)))

    def round_tape_forward_walk(self, field, tape: "RoundTape", inv, entries, n, rounds, checkpoints=None, every=0, cp_stride=0, trace=None,
                                walk_stride=0, base=0, j_base=0, j_walk_step=0) -> None:
        """n walks of `rounds` rounds of a recorded forward body in place over `entries` (device, n x n_adv elements), one lane each;
        strides in entries.  With g = base + r + 1 after round r, walk w writes the entry it produced to trace entry
        w * walk_stride + g and, when every divides g, to checkpoints entry w * cp_stride + g // every (device or None); the round
        sees j = j_base + w * j_walk_step + base + r.  inv: host."""
        self._check(lib.vdf_round_tape_forward_walk(self.handle, field, self._tape(tape), _ptr(inv), _ptr(entries), n, rounds, _ptr(checkpoints),
                                                    every, cp_stride, _ptr(trace), walk_stride, base, j_base, j_walk_step))

    def round_tape_eval_batch(self, field, tape: "RoundTape", inv, initial, n, rounds_total, out_entries, every=0, launch_rounds=0, j_base=0,
                              j_walk_step=0) -> None:
        """Context.minroot_eval_batch for a forward walk tape: out_entries[w] = the final entry of chain w (every = 0), or the
        rounds_total // every + 1 entries it passes every `every` rounds, the initial one first.  initial / out_entries: host or
        device, n_adv elements per entry; inv: host."""
        self._check(lib.vdf_round_tape_eval_batch(self.handle, field, self._tape(tape), _ptr(inv), _ptr(initial), n, rounds_total, every,
                                                  launch_rounds, j_base, j_walk_step, _ptr(out_entries)))

    def minroot_step_segment_packed(self, field, trace_xy, t, i0, i_in, out, packed) -> None:
        """The reference's allocation (4 variables per round) and the 3t + 4 scalars of its commitment without new_x."""
        self._check(lib.vdf_minroot_step_segment_packed(self.handle, field, _ptr(trace_xy), t, _ptr(i0), _ptr(i_in), _ptr(out), _ptr(packed)))

    def minroot_inverse_walk(self, field, states, n, rounds, trace_xy=None, walk_stride=0, top=0, group=0, group_stride=0) -> None:
        """n inverse walks of `rounds` rounds in place over `states` (device, 96 B each); trace_xy (device or None): walk w writes
        the (x, y) it stands on before round r to entry (w // group) * group_stride + (w % group) * walk_stride + top - r."""
        self._check(lib.vdf_minroot_inverse_walk(self.handle, field, _ptr(states), n, rounds, _ptr(trace_xy), walk_stride, top,
                                                 group, group_stride))

    def minroot_check_batch(self, field, results, originals, n, rounds, ok) -> None:
        """ok[w] = 1 iff `rounds` inverse rounds from results[w] land on originals[w]; host or device buffers, ok int32."""
        self._check(lib.vdf_minroot_check_batch(self.handle, field, _ptr(results), _ptr(originals), n, rounds, _ptr(ok)))

    def minroot_trace_heads(self, states, n, state_stride, trace_xy, trace_stride) -> None:
        self._check(lib.vdf_minroot_trace_heads(self.handle, _ptr(states), n, state_stride, _ptr(trace_xy), trace_stride))

    def minroot_forward_walk(self, field, states, n, rounds, checkpoints=None, every=0, cp_stride=0, trace_xy=None, walk_stride=0,
                             base=0) -> None:
        """n forward walks of `rounds` rounds (at most _lib.MINROOT_FORWARD_MAX_ROUNDS) in place over `states` (device, 96 B each).
        With g = base + r + 1 after round r, walk w writes (x, y) to trace entry w * walk_stride + g and, when `every` divides g,
        its state to checkpoints[w * cp_stride + g // every] (device or None).  Many chains at once: throughput, not latency."""
        self._check(lib.vdf_minroot_forward_walk(self.handle, field, _ptr(states), n, rounds, _ptr(checkpoints), every, cp_stride,
                                                 _ptr(trace_xy), walk_stride, base))

    def minroot_eval_batch(self, field, initial, n, rounds_total, out_states, every=0, launch_rounds=0) -> None:
        """vdf_minroot_eval_checkpoints for n chains: out_states[w] = the final state (every = 0), or the rounds_total // every + 1
        states of chain w every `every` rounds, the initial one included; host or device buffers."""
        self._check(lib.vdf_minroot_eval_batch(self.handle, field, _ptr(initial), n, rounds_total, every, launch_rounds, _ptr(out_states)))

    def gate_accumulate(self, other: "Context", slot: int) -> None:
        """The next bucket-method MSM on this context accumulates only after `other`'s mark `slot` (vdf_ctx_gate_accumulate)."""
        self._check(lib.vdf_ctx_gate_accumulate(self.handle, other.handle, slot))

    def set_kernel_timing(self, flag: bool) -> None:
        self._check(lib.vdf_ctx_set_kernel_timing(self.handle, int(flag)))

    def kernel_events(self) -> list:
        """Drains the timed launches of this context: [(kernel, algorithmic bytes, start_ms, end_ms)]."""
        n = C.c_size_t()
        self._check(lib.vdf_ctx_kernel_events(self.handle, None, 0, C.byref(n)))
        ev = np.zeros(n.value + 16, dtype=np.dtype([("name", "S24"), ("bytes", "<f8"), ("start_ms", "<f8"), ("end_ms", "<f8")]))
        self._check(lib.vdf_ctx_kernel_events(self.handle, ev.ctypes.data, ev.shape[0], C.byref(n)))
        return [(ev["name"][i].decode(), float(ev["bytes"][i]), float(ev["start_ms"][i]), float(ev["end_ms"][i])) for i in range(n.value)]

    def vec_is_zero(self, v, n: int) -> bool:
        """True iff all n field elements are zero (decided on the device)."""
        out = C.c_int(0)
        self._check(lib.vdf_vec_is_zero(self.handle, _ptr(v), n, C.byref(out)))
        return bool(out.value)

    def unsat_rows(self, field, az, bz, cz, n: int) -> Tuple[int, int]:
        """(rows r < n with az[r] * bz[r] != cz[r], the smallest of them or 2**64 - 1), decided on the device; az, bz, cz: device
        memory, canonical Montgomery elements."""
        out = (C.c_uint64 * 2)()
        self._check(lib.vdf_unsat_rows(self.handle, field, _ptr(az), _ptr(bz), _ptr(cz), n, out))
        return int(out[0]), int(out[1])

    def nifs_cross_term(self, shape: Shape, z2, az1, bz1, cz1, u1, az2, bz2, cz2, T) -> None:
        self._check(lib.vdf_nifs_cross_term(self.handle, shape.handle, _ptr(z2), _ptr(az1), _ptr(bz1), _ptr(cz1), _ptr(u1),
                                            _ptr(az2), _ptr(bz2), _ptr(cz2), _ptr(T)))

    def nifs_cross_term_rows(self, shape: Shape, row_begin: int, row_count: int, part: int, z2, az1, bz1, cz1, u1, az2, bz2, cz2, T) -> None:
        """part: 1 = only the rows [row_begin, row_begin + row_count), 2 = every row but those (vdf_hip.h VDF_ROWS_*)."""
        self._check(lib.vdf_nifs_cross_term_rows(self.handle, shape.handle, row_begin, row_count, part, _ptr(z2), _ptr(az1), _ptr(bz1),
                                                 _ptr(cz1), _ptr(u1), _ptr(az2), _ptr(bz2), _ptr(cz2), _ptr(T)))

    def nifs_cross_term_minroot(self, field, per, t, seg_begin, one_col, row_begin, z2, az1, bz1, cz1, u1, az2, bz2, cz2, T) -> None:
        """The 3t + 1 rows of a built-in MinRoot step circuit from row_begin on, by stencil (vdf_hip.h)."""
        self._check(lib.vdf_nifs_cross_term_minroot(self.handle, field, per, t, seg_begin, one_col, row_begin, _ptr(z2), _ptr(az1),
                                                    _ptr(bz1), _ptr(cz1), _ptr(u1), _ptr(az2), _ptr(bz2), _ptr(cz2), _ptr(T)))

    def nifs_cross_term_minroot_forward(self, field, t, seg_begin, one_col, row_begin, z2, az1, bz1, cz1, u1, az2, bz2, cz2, T) -> None:
        """The 3t + 1 rows of the forward MinRoot step circuit from row_begin on, by stencil (vdf_hip.h)."""
        self._check(lib.vdf_nifs_cross_term_minroot_forward(self.handle, field, t, seg_begin, one_col, row_begin, _ptr(z2), _ptr(az1),
                                                            _ptr(bz1), _ptr(cz1), _ptr(u1), _ptr(az2), _ptr(bz2), _ptr(cz2), _ptr(T)))

    def nifs_cross_term_minroot_forward_lanes(self, field, t, lanes, seg_begin, one_col, row_begin, z2, az1, bz1, cz1, u1, az2, bz2, cz2, T) -> None:
        """The lanes x (3t + 1) rows of the forward circuit in lanes from row_begin on, by stencil, one launch (vdf_hip.h)."""
        self._check(lib.vdf_nifs_cross_term_minroot_forward_lanes(self.handle, field, t, lanes, seg_begin, one_col, row_begin, _ptr(z2), _ptr(az1),
                                                                  _ptr(bz1), _ptr(cz1), _ptr(u1), _ptr(az2), _ptr(bz2), _ptr(cz2), _ptr(T)))

    def nifs_cross_term_periodic(self, field, rows: "PeriodicRows", j_first, reps, seg_begin, row_begin, num_cols, num_cons, z2, az1, bz1,
                                 cz1, u1, az2, bz2, cz2, T) -> None:
        """Az2, Bz2, Cz2 and T of the rows row_begin + (j - j_first) * n_cons + c, j = j_first .. j_first + reps - 1, from the
        periodic description alone (no sparse matrices); every other row is left as it is.  Vectors: device; u1: host."""
        self._check(lib.vdf_nifs_cross_term_periodic(self.handle, field, C.addressof(rows.c), j_first, reps, seg_begin, row_begin, num_cols,
                                                     num_cons, _ptr(z2), _ptr(az1), _ptr(bz1), _ptr(cz1), _ptr(u1), _ptr(az2), _ptr(bz2),
                                                     _ptr(cz2), _ptr(T)))

    def nifs_cross_term_minroot_fold(self, field, per, t, seg_begin, one_col, row_begin, z2, r, az1, bz1, cz1, e1, t_prev, u1, az2, bz2, cz2, T) -> None:
        """The same rows with the previous fold of those rows applied on the way (vdf_hip.h); e1 / t_prev may be None."""
        self._check(lib.vdf_nifs_cross_term_minroot_fold(self.handle, field, per, t, seg_begin, one_col, row_begin, _ptr(z2), _ptr(r), _ptr(az1),
                                                         _ptr(bz1), _ptr(cz1), _ptr(e1) if e1 is not None else None,
                                                         _ptr(t_prev) if t_prev is not None else None, _ptr(u1), _ptr(az2), _ptr(bz2),
                                                         _ptr(cz2), _ptr(T)))

    def fold_many(self, field, r, acc, add, n) -> None:
        k = len(acc)
        a = (C.c_void_p * k)(*[_ptr(x) for x in acc])
        b = (C.c_void_p * k)(*[_ptr(x) for x in add])
        ln = (C.c_size_t * k)(*[int(x) for x in n])
        self._check(lib.vdf_fold_many(self.handle, field, _ptr(r), k, a, b, ln))

    # ---- compression SNARK building blocks: vectors on the device, scalars as host arrays ----
    def pair_table(self, field, lo, hi, k, out) -> None:
        self._check(lib.vdf_pair_table(self.handle, field, _ptr(lo), _ptr(hi), k, _ptr(out)))

    def pair_table_pattern(self, field, lo, hi, k, pattern, log_m, out) -> None:
        self._check(lib.vdf_pair_table_pattern(self.handle, field, _ptr(lo), _ptr(hi), k, _ptr(pattern), log_m, _ptr(out)))

    def ipa_coefficients(self, field, openings, n, out) -> None:
        """out[i] = sum over the openings of weight * pattern[i mod 2^log_m] * prod_j (bit ? hi[j] : lo[j]) (vdf_hip.h);
        openings: [(weight, lo, hi, pattern)] with Montgomery host arrays of 1, k, k and 2^log_m elements."""
        ops = (IpaOpening * len(openings))()
        keep = []
        for o, (w, lo, hi, pat) in zip(ops, openings):
            lo, hi, pat = (np.ascontiguousarray(x, dtype="<u8").reshape(-1, 4) for x in (lo, hi, pat))
            keep += [lo, hi, pat]
            o.weight = (C.c_uint64 * 4)(*np.ascontiguousarray(w, dtype="<u8").reshape(4).tolist())
            o.k, o.log_m = lo.shape[0], max(pat.shape[0] - 1, 0).bit_length()
            o.lo, o.hi, o.pattern = (x.ctypes.data if x.shape[0] else None for x in (lo, hi, pat))
        self._check(lib.vdf_ipa_coefficients(self.handle, field, ops, len(openings), n, _ptr(out)))

    def fold_halves(self, field, vectors, c_lo, c_hi, n) -> None:
        k = len(vectors)
        v = (C.c_void_p * k)(*[_ptr(x) for x in vectors])
        self._check(lib.vdf_fold_halves(self.handle, field, k, v, _ptr(c_lo), _ptr(c_hi), n))

    def reduce(self, field, kind, tables, n, u=None):
        nout = 1 if kind == 0 else 3 if kind == 2 else 2
        out = np.zeros((nout, 4), dtype="<u8")
        t = (C.c_void_p * len(tables))(*[_ptr(x) for x in tables])
        self._check(lib.vdf_reduce(self.handle, field, kind, t, _ptr(u), n, _ptr(out)))
        return out

    def spmv3_t(self, shape: Shape, eq, rho, out) -> None:
        self._check(lib.vdf_spmv3_t(self.handle, shape.handle, _ptr(eq), _ptr(rho), _ptr(out)))

    def reduce_batch(self, field, kind, tables, n, u=None):
        """vdf_reduce_batch: tables = one list of device vectors per instance (as reduce takes them), u = the instances'
        host elements for kind 2 (count x 4 limbs); returns (count, nout, 4) limbs."""
        count = len(tables)
        nout = 1 if kind == 0 else 3 if kind == 2 else 2
        out = np.zeros((count, nout, 4), dtype="<u8")
        flat = [_ptr(x) for ts in tables for x in ts]
        t = (C.c_void_p * max(len(flat), 1))(*flat)
        if u is not None:
            u = np.ascontiguousarray(u, dtype="<u8").reshape(-1, 4)
        self._check(lib.vdf_reduce_batch(self.handle, field, kind, count, t, _ptr(u), n, _ptr(out)))
        return out

    def fold_halves_batch(self, field, vectors, c_lo, c_hi, n) -> None:
        """vdf_fold_halves_batch: up to 320 vectors of length n, c_lo / c_hi one host element each."""
        k = len(vectors)
        v = (C.c_void_p * max(k, 1))(*[_ptr(x) for x in vectors])
        c_lo, c_hi = (np.ascontiguousarray(x, dtype="<u8").reshape(-1, 4) for x in (c_lo, c_hi))
        self._check(lib.vdf_fold_halves_batch(self.handle, field, k, v, _ptr(c_lo), _ptr(c_hi), n))

    def spmv3_t_batch(self, shape: Shape, eqs, rhos, outs) -> None:
        """vdf_spmv3_t_batch: outs[q] = spmv3_t(eqs[q], rhos[q]) in one pass over the shape's columns."""
        count = len(eqs)
        e = (C.c_void_p * max(count, 1))(*[_ptr(x) for x in eqs])
        o = (C.c_void_p * max(count, 1))(*[_ptr(x) for x in outs])
        r = np.ascontiguousarray(rhos, dtype="<u8").reshape(-1, 4)
        self._check(lib.vdf_spmv3_t_batch(self.handle, shape.handle, count, e, _ptr(r), o))

    def lincomb_u128(self, field, vectors, lengths, weights, n_out, out) -> None:
        """vdf_lincomb_u128: out[i] = sum_j weights[j] * vectors[j][i] (zero past lengths[j]); weights: plain integers below
        2^128 as a (count, 4) uint64 host array."""
        count = len(vectors)
        v = (C.c_void_p * max(count, 1))(*[_ptr(x) for x in vectors])
        ln = (C.c_size_t * max(count, 1))(*[int(x) for x in lengths])
        w = np.ascontiguousarray(weights, dtype="<u8").reshape(-1, 4)
        self._check(lib.vdf_lincomb_u128(self.handle, field, count, v, ln, _ptr(w), n_out, _ptr(out)))

    def relaxed_residual_batch(self, shape: Shape, zs, Es, us, rhos, out) -> None:
        """vdf_relaxed_residual_batch: out[r] = sum_q rhos[q] ((A z_q)[r] (B z_q)[r] - us[q] (C z_q)[r] - Es[q][r]); an E of None
        is zero; us Montgomery, rhos plain integers below 2^128, both (count, 4) uint64 host arrays."""
        count = len(zs)
        z = (C.c_void_p * max(count, 1))(*[_ptr(x) for x in zs])
        e = (C.c_void_p * max(count, 1))(*[None if x is None else _ptr(x) for x in Es])
        u = np.ascontiguousarray(us, dtype="<u8").reshape(-1, 4)
        r = np.ascontiguousarray(rhos, dtype="<u8").reshape(-1, 4)
        self._check(lib.vdf_relaxed_residual_batch(self.handle, shape.handle, count, z, e, _ptr(u), _ptr(r), _ptr(out)))

    def sparse_eval_multi(self, shape: Shape, eq_xs, eq_ys, rhos, col_split=None, col_hi_base=0, out=None):
        """vdf_sparse_eval_multi: out[q] = sum over the entries (x, y, v) of A, B, C of eq_xs[q][x] w_q v eq_ys[q][ycol(y)], w_q = 1,
        rhos[q], rhos[q]^2, for all q in one pass over the rows; ycol(y) = y below col_split (default: num_cols, the identity), else
        col_hi_base + (y - col_split).  eq_xs, eq_ys: device tensors of (nx, 4) and (ny, 4) uint64 limbs, Montgomery, one length
        each; rhos: (count, 4) Montgomery host limbs.  Returns the (count, 4) limbs (a host array; `out` if given)."""
        count = len(eq_xs)
        if len(eq_ys) != count:
            raise ValueError("one column vector per row vector")
        nx = {int(x.shape[0]) for x in eq_xs}
        ny = {int(y.shape[0]) for y in eq_ys}
        if len(nx) > 1 or len(ny) > 1:
            raise ValueError("the vectors of a call have one length")
        ex = (C.c_void_p * max(count, 1))(*[_ptr(x) for x in eq_xs])
        ey = (C.c_void_p * max(count, 1))(*[_ptr(y) for y in eq_ys])
        r = np.ascontiguousarray(rhos, dtype="<u8").reshape(-1, 4)
        if r.shape[0] != count:
            raise ValueError("one rho per instance")
        if out is None:
            out = np.zeros((count, 4), dtype="<u8")
        split = shape.num_cols if col_split is None else col_split
        self._check(lib.vdf_sparse_eval_multi(self.handle, shape.handle, count, ex, nx.pop() if nx else 0, ey, ny.pop() if ny else 0,
                                              _ptr(r), split, col_hi_base, _ptr(out)))
        return out

    def ipa_scalars(self, field, a, s, n, nj, sL, sR) -> None:
        self._check(lib.vdf_ipa_scalars(self.handle, field, _ptr(a), _ptr(s), n, nj, _ptr(sL), _ptr(sR)))

    def scale_pattern(self, field, s, n, nj, x_lo, x_hi) -> None:
        self._check(lib.vdf_scale_pattern(self.handle, field, _ptr(s), n, nj, _ptr(x_lo), _ptr(x_hi)))

    def fe_mul(self, field, a, b, n, out) -> None:
        self._check(lib.vdf_fe_mul(self.handle, field, _ptr(a), _ptr(b), n, _ptr(out)))

    def fe_to_mont(self, field, a, n, out) -> None:
        self._check(lib.vdf_fe_to_mont(self.handle, field, _ptr(a), n, _ptr(out)))

    def fe_from_mont(self, field, a, n, out) -> None:
        self._check(lib.vdf_fe_from_mont(self.handle, field, _ptr(a), n, _ptr(out)))

    def fe_sqrt(self, field, a, n, out, ok) -> None:
        """vdf_fe_sqrt: out[i] = the root of a[i] whose canonical value is even and ok[i] = 1, or zero and ok[i] = 0 for a
        non-residue; a, out: (n, 4) uint64 Montgomery limbs, ok: n uint8; numpy arrays or device tensors, each on its own."""
        self._check(lib.vdf_fe_sqrt(self.handle, field, _ptr(a), n, _ptr(out), _ptr(ok)))

    def points_decompress(self, curve, enc, n, out, ok) -> None:
        """vdf_points_decompress: n points from their 32-byte wire encodings; enc: n x 32 uint8, out: (n, 8) uint64 Montgomery
        limbs (x, y), ok: n uint8 (0: the bytes decode to no point, out zeroed); numpy arrays or device tensors, each on its own."""
        self._check(lib.vdf_points_decompress(self.handle, curve, _ptr(enc), n, _ptr(out), _ptr(ok)))

    def points_axpy(self, curve, a, b, s, bits, n, out) -> None:
        """vdf_points_axpy: out[i] = a[i] + s[i] b[i]; a, b, out: (n, 8) uint64 affine points in Montgomery form (the identity
        is all zero), s: (n, 4) uint64 plain little-endian integers of which the low `bits` (128 or 255) count and the rest is
        masked; numpy arrays or device tensors, each on its own."""
        self._check(lib.vdf_points_axpy(self.handle, curve, _ptr(a), _ptr(b), _ptr(s), bits, n, _ptr(out)))

    def ro_hash_batch(self, field, tag, rc, xs, len, n, bits, out) -> None:
        """vdf_ro_hash_batch: the family-0 random oracle of n messages of `len` elements each (message-major Montgomery limbs),
        one lane per message; rc: the field's 88 round constants (nova.ro_constants); out: (n, 4) uint64 -- bits = 0: the element
        in Montgomery form, 1..255: the low bits of its canonical integer as a plain integer.  Each array in host or device
        memory."""
        self._check(lib.vdf_ro_hash_batch(self.handle, field, tag, _ptr(rc), _ptr(xs), len, n, bits, _ptr(out)))

    def ro_hash_batch_block(self, field, tag, width, full_rounds, partial_rounds, rc, mds, xs, len, n, bits, out) -> None:
        """vdf_ro_hash_batch_block: the family-1 random oracle (width, full_rounds, partial_rounds; rate width - 1) of n messages
        of `len` elements each, one message per 32 lanes; rc, mds: the block's round constants and matrix (nova.ro_block_constants);
        xs, bits and out as ro_hash_batch.  Each array in host or device memory."""
        self._check(lib.vdf_ro_hash_batch_block(self.handle, field, tag, width, full_rounds, partial_rounds, _ptr(rc), _ptr(mds), _ptr(xs),
                                                len, n, bits, _ptr(out)))

    def clock_probe(self, iters: int = 6000):
        """(shader MHz sustained under a multiply-bound load on every SIMD, the probe kernel's duration in ms)."""
        mhz, ms = C.c_double(), C.c_double()
        self._check(lib.vdf_ctx_clock_probe(self.handle, iters, C.byref(mhz), C.byref(ms)))
        return mhz.value, ms.value

    def fe_mul_chain(self, field, a, n, iters, out) -> None:
        self._check(lib.vdf_fe_mul_chain(self.handle, field, _ptr(a), n, iters, _ptr(out)))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
