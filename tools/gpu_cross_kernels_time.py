#!/usr/bin/env python3
"""Every cross-term kernel alone at t = 2^16 on one MI355X, profiler off: per-launch HIP events (vdf_ctx_kernel_events), 41 launches
each, the first dropped; one line per (arrangement, kernel) with median, min and max in us (profiles/r23_cross_operands.txt).

  python tools/gpu_cross_kernels_time.py TAG        TAG labels the lines; VDF_HIP_LIB=<path> times another build of the library

Shapes: circuit F of tests/rounds_spec.py (its augmented primary shape) for the sparse kernels in every lane count and for the
periodic rows; vectors of the built-in kinds' sizes for the inverse, forward and fold stencils (values arbitrary: only the time
counts, but for one = 1, the prover's case)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import vdf_amd
from vdf_amd import hip
from rounds_spec import F
from vdf_amd.minroot import FIELD_FQ, State
from vdf_amd.nova import shape_export_custom, shape_periodic_custom

tag, launches, t = (sys.argv[1] if len(sys.argv) > 1 else "this"), 41, 1 << 16
ctx = vdf_amd.Context(0)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
rng = np.random.default_rng(16)


def rand(n):
    v = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return v


ONE = np.frombuffer(State.from_ints(FIELD_FQ, 1, 0, 0).x, dtype="<u8")
circuit = F(t, "repeat")
mats = shape_export_custom(circuit)
pr, info = shape_periodic_custom(circuit)
nc, ncols = info["num_cons"], info["num_cols"]
shape = ctx.shape_create(FIELD_FQ, nc, ncols, mats)
z2 = rand(ncols)
z2[ncols - 3] = ONE
d_in = [dev(z2)] + [dev(rand(nc)) for _ in range(3)]
u1 = rand(1)
outs = [torch.zeros((nc, 4), dtype=torch.int64, device="cuda") for _ in range(4)]
reps = t - pr.lead
# the stencils: 4 t + 1 round variables behind z_in, the constant right behind them; 3 t + 1 rows
sn, sc = 3 * t + 1 + 8, 3 + 4 * t + 1 + 9
sz = rand(sc)
one_col = 3 + 4 * t + 1
sz[one_col] = ONE
s_in = [dev(sz)] + [dev(rand(sn)) for _ in range(3)]
s_out = [dev(rand(sn)) for _ in range(4)]
s_e = dev(rand(sn))
r128 = np.zeros((1, 4), dtype="<u8")
r128[0, :2] = rng.integers(1, 2**63, size=2, dtype=np.uint64)
r_m = np.frombuffer(State.from_ints(FIELD_FQ, int(r128[0, 0]) | int(r128[0, 1]) << 64, 0, 0).x, dtype="<u8").reshape(1, 4).copy()


def tuned(lanes, fused, f):
    def g():
        base = hip.tuning_get()
        hip.tuning_set(nifs_lanes=lanes, nifs_fused=fused)
        try:
            f()
        finally:
            import ctypes
            hip.lib.vdf_hip_tuning_set(ctypes.byref(base))
    return g


outside = lambda: ctx.nifs_cross_term_rows(shape, pr.row_begin, pr.row_count, 2, *d_in, u1, *outs)
variants = {
    "all rows, lane per row": lambda: ctx.nifs_cross_term(shape, *d_in, u1, *outs),
    "outside, fused 8 lanes": tuned(0, 1, outside),
    "outside, unfused 8 lanes": tuned(8, 0, outside),
    "all rows, 4 lanes": tuned(4, 0, lambda: ctx.nifs_cross_term(shape, *d_in, u1, *outs)),
    "periodic": lambda: ctx.nifs_cross_term_periodic(FIELD_FQ, pr, pr.lead, reps, info["seg_begin"], pr.row_begin, ncols, nc, *d_in, u1, *outs),
    "inverse stencil, 4 per round": lambda: ctx.nifs_cross_term_minroot(FIELD_FQ, 4, t, 3, one_col, 0, *s_in, u1, *s_out),
    "inverse stencil, 3 per round": lambda: ctx.nifs_cross_term_minroot(FIELD_FQ, 3, t, 3, one_col, 0, *s_in, u1, *s_out),
    "forward stencil": lambda: ctx.nifs_cross_term_minroot_forward(FIELD_FQ, t, 3, one_col, 0, *s_in, u1, *s_out),
    "fold stencil, 4 per round, E": lambda: ctx.nifs_cross_term_minroot_fold(FIELD_FQ, 4, t, 3, one_col, 0, s_in[0], r_m, *s_in[1:], s_e, s_out[3], u1, *s_out),
    "fold stencil, 3 per round, E": lambda: ctx.nifs_cross_term_minroot_fold(FIELD_FQ, 3, t, 3, one_col, 0, s_in[0], r_m, *s_in[1:], s_e, s_out[3], u1, *s_out),
}
for f in variants.values():
    f()
ctx.sync()
ctx.set_kernel_timing(True)
ctx.kernel_events()
times = {}
for _ in range(launches):
    for k, f in variants.items():
        f()
        ctx.sync()
        for name, _b, t0, t1 in ctx.kernel_events():
            times.setdefault((k, name), []).append((t1 - t0) * 1e3)
for (k, name), d in times.items():
    d = d[1:]
    print("[%s] %-30s %-24s us per launch over %d: median %8.2f  min %8.2f  max %8.2f" % (tag, k, name, len(d), statistics.median(d), min(d), max(d)),
          flush=True)
shape.free()
ctx.close()
