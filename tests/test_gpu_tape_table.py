"""GPU: VDF_TAPE_TAB on the device (include/vdf_hip.h; tests/tab_spec.py states it as integers, tests/test_tape_table_host.py checks
the host evaluators against that).  Every device result is compared with the host evaluator of the same call, byte for byte.

a. the round kernels (k_round_tape_tab, k_round_tape_lanes_tab): t around the wavefront boundary x rows that are and are not powers
   of two; lanes 1, 3, 16 with an inv per lane;
b. the descending walks (k_tape_walk_tab, k_tape_walk_lanes_tab): one walk and more than a wavefront x 1, 2, 7 rounds; the chain
   layout with heads, expect and ok; rows = 3 under j_base = 2^64 - 5, J crossing the wrap inside a walk; two lanes whose j_base
   differ modulo rows;
c. the forward walks (k_tape_forward_walk_tab): TAB with POW, TAB with POWC, eval_batch cut so that base != 0 enters J, the wrap
   ascending;
d. an oracle that is not this change: over a table whose entry r is i0 + r the tabbed forward tape is vdf_minroot_eval_batch and the
   tabbed walk tape vdf_minroot_inverse_walk, in both fields;
e. a tape without a TAB launches the old kernels and writes the old bytes; a tabbed tape launches the new ones; a table that is
   not device-readable is refused;
f. proofs of the tabbed MinRoot round at t = 8, rows = 4, 3 steps: host advice, device advice and the chain from checkpoints give
   the same bytes, under every custom_ahead and with periodic_rows = 1, in two lanes and over Fp; the refusals and the wrong tables;
g. examples/prove_tabbed_chain as a fresh child process."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import tab_spec as ts
from rounds_spec import MOD, mont_rows
from util import dev, host, mont_states
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import TAPE_TAB, VdfError
from vdf_amd.minroot import pow_chain as minroot_pow_chain
from vdf_amd.nova import (CustomChain, NovaVDFProof, forward_tape_eval, public_params_custom, record_forward_body, record_round_body,
                          record_walk_body, round_tape_eval, round_tape_eval_lanes, shape_digest_custom, walk_tape_eval,
                          walk_tape_eval_lanes, FIELD_FP, FIELD_FQ)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [1, 3, 64, 65]
COLS = 8


def zeros(n):
    import torch
    return torch.zeros((n, 4), dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def table(rows, cols, field):
    m = MOD[field]
    vals = ts.table_ints(rows, cols, m)
    return vals, ts.table_array(vals, rows, cols, m)


@functools.lru_cache(maxsize=None)
def tape_of(kind, rows, field, chain=False):
    """one tape per (kind, rows, field) for the whole module: a context places a tape's table on the device once"""
    _, T = table(rows, COLS, field)
    if kind == "round":
        return record_round_body(ts.round_body(field, T, 0, COLS - 1), field)
    if kind == "walk":
        return record_walk_body(ts.walk_body(field, T, 0, COLS - 1), field)
    return record_forward_body(ts.forward_body(field, T, 0, COLS - 1, chain=chain), field)


def starts(n, m, seed):
    vals = [int(v) for v in np.random.default_rng(seed).integers(1, 2**62, size=n * 3)]
    vals[1 % len(vals)], vals[-1] = 0, m - 1
    return vals


# ---- a. the round kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("t", [1, 63, 64, 65, 130])
def test_the_round_kernel_is_the_host_evaluator(ctx, t, rows):
    field = FIELD_FQ if (t + rows) % 2 else FIELD_FP
    m = MOD[field]
    vals, _ = table(rows, COLS, field)
    tape = tape_of("round", rows, field)
    adv = mont_rows(ts.round_advice(5, 9, t, m, np.random.default_rng(t), vals, rows, COLS, 0, COLS - 1), m)
    inv = mont_rows([9], m)
    want = round_tape_eval(field, tape, t, inv, adv)
    d_out = zeros(t * tape.c.n_vars)
    ctx.round_tape_run(field, tape, t, inv, dev(adv), d_out)
    ctx.sync()
    assert host(d_out).tobytes() == want.tobytes()


@pytest.mark.parametrize("lanes", [1, 3, 16])
def test_the_round_kernel_in_lanes_is_the_host_evaluator(ctx, lanes):
    field, t, rows = FIELD_FQ, 65, 3
    m = MOD[field]
    vals, _ = table(rows, COLS, field)
    tape = tape_of("round", rows, field)
    rng = np.random.default_rng(lanes)
    ks = [(7 + 1000 * l) % m for l in range(lanes)]                 # another inv per lane
    stride, flat = t + 2, []
    for l in range(lanes):
        flat += ts.round_advice(5 + l, ks[l], t, m, rng, vals, rows, COLS, 0, COLS - 1) + [0] * 3
    adv, inv = mont_rows(flat, m), mont_rows(ks, m)
    want = round_tape_eval_lanes(field, tape, t, lanes, inv, adv, stride)
    d_out = zeros(lanes * t * tape.c.n_vars)
    ctx.round_tape_run_lanes(field, tape, t, lanes, inv, dev(adv), stride, d_out)
    ctx.sync()
    assert host(d_out).tobytes() == want.tobytes()


# ---- b. the descending walks ---------------------------------------------------------------------------------------------------
def walk_both(ctx, field, tape, inv, start, n, rounds, trace_entries=0, expect=None, lanes=0, **kw):
    """the same call on the host and on the device: (entries, trace, ok) of both, as bytes"""
    e = start.copy()
    tr = np.zeros((trace_entries * 3, 4), dtype="<u8") if trace_entries else None
    ok = np.full(n, -7, dtype="<i4") if expect is not None else None
    d_e, d_tr = dev(start), zeros(trace_entries * 3) if trace_entries else None
    d_ok = None
    if expect is not None:
        import torch
        d_ok = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    if lanes:
        walk_tape_eval_lanes(field, tape, lanes, inv, e, n, rounds, trace=tr, expect=expect, ok=ok, **kw)
        ctx.round_tape_walk_lanes(field, tape, lanes, inv, d_e, n, rounds, trace=d_tr, expect=None if expect is None else dev(expect), ok=d_ok, **kw)
    else:
        walk_tape_eval(field, tape, inv, e, n, rounds, trace=tr, expect=expect, ok=ok, **kw)
        ctx.round_tape_walk(field, tape, inv, d_e, n, rounds, trace=d_tr, expect=None if expect is None else dev(expect), ok=d_ok, **kw)
    ctx.sync()
    got = (host(d_e).tobytes(), host(d_tr).tobytes() if trace_entries else None, d_ok.cpu().numpy().tolist() if expect is not None else None)
    return (e.tobytes(), tr.tobytes() if trace_entries else None, ok.tolist() if expect is not None else None), got


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("rounds", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 65])
def test_the_walk_kernel_is_the_host_evaluator(ctx, n, rounds, rows):
    field = FIELD_FQ if (n + rounds + rows) % 2 else FIELD_FP
    m = MOD[field]
    start = mont_rows(starts(n, m, rows + rounds), m)
    want, got = walk_both(ctx, field, tape_of("walk", rows, field), mont_rows([99], m), start, n, rounds, trace_entries=n * 8, walk_stride=8,
                          top=7, j_base=1000003)
    assert got == want


@pytest.mark.parametrize("rows", [3, 4])
def test_the_chain_layout_with_heads_expect_and_ok(ctx, rows):
    """t = 8, every = 4, 3 steps: 6 walks in 3 groups of 2, traces of 9 entries back to back, J chain-global; the targets are the
    landings themselves but for walk 4's"""
    field, t, every, steps = FIELD_FQ, 8, 4, 3
    m = MOD[field]
    tape, inv = tape_of("walk", rows, field), mont_rows([99], m)
    start = mont_rows(starts(6, m, 1), m)
    lay = dict(walk_stride=every, top=every, group=t // every, group_stride=t + 1, j_base=16, j_group_step=t, heads=True)
    land = start.copy()
    walk_tape_eval(field, tape, inv, land, 6, every, **lay)
    land[3 * 4 + 1, 0] ^= np.uint64(1)
    want, got = walk_both(ctx, field, tape, inv, start, 6, every, trace_entries=steps * (t + 1), expect=land, **lay)
    assert got == want and want[2] == [1, 1, 1, 1, 0, 1]


@pytest.mark.parametrize("n", [2, 65])
def test_a_walk_whose_counter_crosses_the_wrap(ctx, n):
    """rows = 3 under j_base = 2^64 - 5: 2^64 is no multiple of 3, so a row stepped down across the wrap without taking the
    remainder again would be off by one from there on"""
    field, rows = FIELD_FQ, 3
    m = MOD[field]
    assert 2**64 % rows != 0
    start = mont_rows(starts(n, m, 2), m)
    for j_base in (2**64 - 5, 2**64 - 1, 0):                       # J runs 2^64 + 1 .. 2^64 - 5, 2^64 + 5 .. 2^64 - 1, 6 .. 0
        want, got = walk_both(ctx, field, tape_of("walk", rows, field), mont_rows([99], m), start, n, 7, trace_entries=n * 8, walk_stride=8,
                              top=7, j_base=j_base)
        assert got == want, j_base
    # the spec agrees with both (the host evaluator is checked against it on the CPU; this pins the case itself)
    vals, _ = table(rows, COLS, field)
    land = starts(n, m, 2)
    ts.model_walk(lambda cur, J, inv, mm: ts.walk_ints(cur, J, inv, mm, vals, rows, COLS, 0, COLS - 1), m, 3, [99], land, n, 7,
                  walk_stride=8, top=7, j_base=2**64 - 5)
    want, _ = walk_both(ctx, field, tape_of("walk", rows, field), mont_rows([99], m), start, n, 7, walk_stride=8, top=7, j_base=2**64 - 5)
    assert want[0] == mont_rows(land, m).tobytes()


@pytest.mark.parametrize("rows", [3, 65])
def test_two_lanes_whose_j_base_differ_modulo_the_rows(ctx, rows):
    field = FIELD_FP
    m = MOD[field]
    n, every, t = 8, 4, 8                                          # 2 steps x 2 lanes x 2 intervals
    start = mont_rows(starts(n, m, 3), m)
    jb = [2**64 - 3, 8]
    assert jb[0] % rows != jb[1] % rows
    want, got = walk_both(ctx, field, tape_of("walk", rows, field), mont_rows([99, 98], m), start, n, every, trace_entries=4 * (t + 1), lanes=2,
                          walk_stride=every, top=every, group=t // every, group_stride=t + 1, j_base=jb, j_group_step=t, heads=True)
    assert got == want


# ---- c. the forward walks ------------------------------------------------------------------------------------------------------
def forward_both(ctx, field, tape, inv, start, n, rounds, cp_entries=0, trace_entries=0, **kw):
    e = start.copy()
    cp = np.zeros((cp_entries * 3, 4), dtype="<u8") if cp_entries else None
    tr = np.zeros((trace_entries * 3, 4), dtype="<u8") if trace_entries else None
    forward_tape_eval(field, tape, inv, e, n, rounds, checkpoints=cp, trace=tr, **kw)
    d_e, d_cp, d_tr = dev(start), zeros(cp_entries * 3) if cp_entries else None, zeros(trace_entries * 3) if trace_entries else None
    ctx.round_tape_forward_walk(field, tape, inv, d_e, n, rounds, checkpoints=d_cp, trace=d_tr, **kw)
    ctx.sync()
    return ((e.tobytes(), cp.tobytes() if cp_entries else None, tr.tobytes() if trace_entries else None),
            (host(d_e).tobytes(), host(d_cp).tobytes() if cp_entries else None, host(d_tr).tobytes() if trace_entries else None))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("chain", [False, True], ids=["pow", "pow and powc"])
@pytest.mark.parametrize("n", [1, 65])
def test_the_forward_kernel_is_the_host_evaluator(ctx, n, chain, rows):
    field = FIELD_FQ if (n + rows) % 2 else FIELD_FP
    m = MOD[field]
    tape = tape_of("forward", rows, field, chain)
    assert (10 in {x[0] for x in tape.op_list()}) == chain and {9, TAPE_TAB} <= {x[0] for x in tape.op_list()}
    start = mont_rows(starts(n, m, rows), m)
    want, got = forward_both(ctx, field, tape, mont_rows([99], m), start, n, 7, cp_entries=n * 4, trace_entries=n * 11, every=3, cp_stride=4,
                             walk_stride=11, base=2, j_base=1000003, j_walk_step=1000)
    assert got == want


@pytest.mark.parametrize("n", [2, 65])
def test_a_forward_walk_whose_counter_crosses_the_wrap(ctx, n):
    field, rows = FIELD_FQ, 3
    m = MOD[field]
    start = mont_rows(starts(n, m, 4), m)
    for j_base in (2**64 - 5, 2**64 - 7, 2**64 - 1):
        want, got = forward_both(ctx, field, tape_of("forward", rows, field), mont_rows([99], m), start, n, 7, trace_entries=n * 8, walk_stride=8,
                                 j_base=j_base)
        assert got == want, j_base
    vals, _ = table(rows, COLS, field)
    land = starts(n, m, 4)
    ts.model_forward(lambda cur, J, inv, mm: ts.forward_ints(cur, J, inv, mm, vals, rows, COLS, 0, COLS - 1), m, 3, [99], land, n, 7,
                     j_base=2**64 - 5)
    want, _ = forward_both(ctx, field, tape_of("forward", rows, field), mont_rows([99], m), start, n, 7, j_base=2**64 - 5)
    assert want[0] == mont_rows(land, m).tobytes()


@pytest.mark.parametrize("rows", [3, 64])
def test_eval_batch_cut_into_launches_so_that_base_enters_the_counter(ctx, rows):
    """rounds_total = 8, every = 4, launch_rounds = 3: launches of 3, 3 and 2 rounds, the second and third with base 3 and 6"""
    field, n = FIELD_FP, 5
    m = MOD[field]
    tape, inv = tape_of("forward", rows, field), mont_rows([99], m)
    start = mont_rows(starts(n, m, 5), m)
    e, cps = start.copy(), np.zeros((n * 3 * 3, 4), dtype="<u8")
    cps.reshape(n, 3, 3, 4)[:, 0] = start.reshape(n, 3, 4)
    forward_tape_eval(field, tape, inv, e, n, 8, checkpoints=cps, every=4, cp_stride=3, j_base=2**64 - 4, j_walk_step=7)
    out = np.zeros_like(cps)
    ctx.round_tape_eval_batch(field, tape, inv, start, n, 8, out, every=4, launch_rounds=3, j_base=2**64 - 4, j_walk_step=7)
    ctx.sync()
    assert out.tobytes() == cps.tobytes()


# ---- d. an oracle that does not come from this change --------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_over_a_table_of_counters_the_tabbed_tapes_are_minroot(ctx, field):
    m, rows, rounds, i0, n = MOD[field], 64, 64, 1234567, 3
    vals = [(i0 + r) % m for r in range(rows)]
    T = ts.table_array(vals, rows, 1, m)
    fwd = record_forward_body(ts.minroot_forward_body(field, T, None, 0, minroot_pow_chain(field)), field)
    back = record_walk_body(ts.minroot_walk_body(field, T, None, 0), field)
    xy = [5, 0, 6, 11, m - 1, 0]
    first = mont_states([(xy[2 * w], xy[2 * w + 1], i0) for w in range(n)], m)
    last = np.zeros_like(first)
    ctx.minroot_eval_batch(field, first, n, rounds, last)
    d_e = dev(mont_rows(xy, m))
    ctx.round_tape_forward_walk(field, fwd, None, d_e, n, rounds)
    ctx.sync()
    assert host(d_e).tobytes() == np.ascontiguousarray(last.reshape(n, 3, 4)[:, :2]).tobytes()
    # back down: the built-in inverse walk from the same states, the tabbed walk tape from their (x, y); J of the last round is 63
    d_s = dev(last)
    ctx.minroot_inverse_walk(field, d_s, n, rounds)
    ctx.round_tape_walk(field, back, None, d_e, n, rounds, top=rounds)
    ctx.sync()
    assert host(d_s).tobytes() == first.tobytes()
    assert host(d_e).tobytes() == mont_rows(xy, m).tobytes()


# ---- e. which kernels run ------------------------------------------------------------------------------------------------------
def test_a_tape_without_a_table_runs_the_old_kernels_and_a_tabbed_one_the_new(ctx):
    from forward_tape_spec import every_op_forward_body
    from rounds_spec import G
    from walks_spec import every_op_body
    field = FIELD_FQ
    m = MOD[field]
    inv, start = mont_rows([99], m), mont_rows(starts(2, m, 6), m)
    old_r, old_w, old_f = record_round_body(G(4, "repeat").body(), field), record_walk_body(every_op_body(field), field), \
        record_forward_body(every_op_forward_body(field), field)
    assert all(t.c.tab_rows == 0 and t.table is None for t in (old_r, old_w, old_f))
    adv = mont_rows(G.advice_for(5, 9, 4, m, np.random.default_rng(1)), m)
    vals, _ = table(3, COLS, field)
    tadv = mont_rows(ts.round_advice(5, 9, 4, m, np.random.default_rng(1), vals, 3, COLS, 0, COLS - 1), m)
    try:
        ctx.set_kernel_timing(True)
        ctx.kernel_events()
        outs = []
        for rt, a in ((old_r, adv), (tape_of("round", 3, field), tadv)):
            d_out = zeros(4 * rt.c.n_vars)
            ctx.round_tape_run(field, rt, 4, mont_rows([9], m), dev(a), d_out)
            d_out2 = zeros(4 * rt.c.n_vars)
            ctx.round_tape_run_lanes(field, rt, 4, 1, mont_rows([9], m), dev(a), 5, d_out2)
            outs.append((rt, a, d_out, d_out2))
        walks = []
        for wt in (old_w, tape_of("walk", 3, field)):
            d_e, d_e2 = dev(start), dev(start)
            ctx.round_tape_walk(field, wt, inv, d_e, 2, 3, j_base=5)
            ctx.round_tape_walk_lanes(field, wt, 1, inv, d_e2, 2, 3, j_base=[5])
            walks.append((wt, d_e, d_e2))
        fwds = []
        for ft in (old_f, tape_of("forward", 3, field), tape_of("forward", 3, field, True)):
            d_e = dev(start)
            ctx.round_tape_forward_walk(field, ft, inv, d_e, 2, 3, j_base=5)
            fwds.append((ft, d_e))
        ctx.sync()
        names = [e[0] for e in ctx.kernel_events()]
    finally:
        ctx.set_kernel_timing(False)
    assert names == ["k_round_tape", "k_round_tape_lanes", "k_round_tape_tab", "k_round_tape_lanes_tab", "k_tape_walk", "k_tape_walk_lanes",
                     "k_tape_walk_tab", "k_tape_walk_lanes_tab", "k_tape_forward_walk", "k_tape_forward_walk_tab", "k_tape_forward_walk_tab"]
    for rt, a, d_out, d_out2 in outs:
        want = round_tape_eval(field, rt, 4, mont_rows([9], m), a).tobytes()
        assert host(d_out).tobytes() == want and host(d_out2).tobytes() == want
    for wt, d_e, d_e2 in walks:
        e = start.copy()
        walk_tape_eval(field, wt, inv, e, 2, 3, j_base=5)
        assert host(d_e).tobytes() == e.tobytes() and host(d_e2).tobytes() == e.tobytes()
    for ft, d_e in fwds:
        e = start.copy()
        forward_tape_eval(field, ft, inv, e, 2, 3, j_base=5)
        assert host(d_e).tobytes() == e.tobytes()


def test_a_table_in_plain_host_memory_is_refused_by_every_launcher(ctx):
    """the category of `a device pointer where host memory is read or the reverse`: a kernel reads the table in place"""
    import ctypes as C
    from vdf_amd._lib import lib
    field = FIELD_FQ
    m = MOD[field]
    d = dev(mont_rows(list(range(1, 31)), m))
    d_out = zeros(64)
    jb = np.zeros(1, dtype="<u8")
    inv = mont_rows([9], m)
    r, w, f = (C.addressof(tape_of(k, 3, field).c) for k in ("round", "walk", "forward"))      # `c` names the numpy table
    calls = [lambda: lib.vdf_round_tape_run(ctx.handle, field, r, 2, inv.ctypes.data, d.data_ptr(), d_out.data_ptr()),
             lambda: lib.vdf_round_tape_run_lanes(ctx.handle, field, r, 2, 1, inv.ctypes.data, d.data_ptr(), 3, d_out.data_ptr()),
             lambda: lib.vdf_round_tape_walk(ctx.handle, field, w, inv.ctypes.data, d.data_ptr(), 1, 1, None, 0, 0, 0, 0, 0, 0, 0, None, None),
             lambda: lib.vdf_round_tape_walk_lanes(ctx.handle, field, w, 1, inv.ctypes.data, d.data_ptr(), 1, 1, None, 0, 0, 0, 0, jb.ctypes.data, 0, 0, None, None),
             lambda: lib.vdf_round_tape_forward_walk(ctx.handle, field, f, inv.ctypes.data, d.data_ptr(), 1, 1, None, 0, 0, None, 0, 0, 0, 0),
             lambda: lib.vdf_round_tape_eval_batch(ctx.handle, field, f, inv.ctypes.data, d.data_ptr(), 1, 1, 0, 0, 0, 0, d_out.data_ptr())]
    before = host(d).tobytes()
    for call in calls:
        assert call() == VDF_ERR_BAD_ARG
        assert b"table" in lib.vdf_last_error(ctx.handle)
    ctx.sync()
    assert host(d).tobytes() == before and not host(d_out).any()


def test_a_tape_given_another_table_is_placed_anew_and_a_collected_tape_frees_its_copy(ctx):
    """RoundTape.set_table around device calls: a larger table (the old copy would be read far past its end), a table of the same
    size with other values (the old copy would answer), dimensions patched past the copy; and the copy of a tape nobody holds"""
    import gc
    import weakref
    field = FIELD_FQ
    m = MOD[field]
    start, inv = mont_rows(starts(65, m, 9), m), mont_rows([99], m)

    def both(tape, j_base):
        e, d_e = start.copy(), dev(start)
        walk_tape_eval(field, tape, inv, e, 65, 7, j_base=j_base)
        ctx.round_tape_walk(field, tape, inv, d_e, 65, 7, j_base=j_base)
        ctx.sync()
        return e.tobytes(), host(d_e).tobytes()
    small_vals = ts.table_ints(3, 2, m)
    small = ts.table_array(small_vals, 3, 2, m)
    tape = record_walk_body(ts.walk_body(field, small, 0, 1), field)
    want, got = both(tape, 5)
    assert got == want
    before = len(ctx._tape_tables)
    big = ts.table_array(ts.table_ints(4096, 2, m), 4096, 2, m)               # 256 KiB where the first copy has 192 bytes
    tape.set_table(big)
    want2, got2 = both(tape, 4090)                                           # rows 4089 .. 4095 and 0 .. 6 over the 65 walks' rounds
    assert got2 == want2 and want2 != want
    other = ts.table_array([v + 1 for v in small_vals], 3, 2, m)             # the first table's size, other values
    tape.set_table(other)
    want3, got3 = both(tape, 5)
    assert got3 == want3 and want3 != want
    assert len(ctx._tape_tables) == before                                   # one copy per tape: the replaced ones are gone
    tape.c.tab_rows = 4                                                      # dimensions past the copy never reach a kernel
    with pytest.raises(ValueError):
        ctx.round_tape_walk(field, tape, inv, dev(start), 65, 7)
    tape.c.tab_rows = 3
    assert both(tape, 5) == (want3, want3)
    ref = weakref.ref(tape)
    del tape
    gc.collect()
    assert ref() is None and len(ctx._tape_tables) == before - 1


# ---- f. proofs -----------------------------------------------------------------------------------------------------------------
T_, EVERY, STEPS, PROWS, X0 = 8, 4, 3, 4, 0x51DE
_PP = {}


@pytest.fixture(scope="module", autouse=True)
def free_the_parameter_sets():
    yield
    for pp in _PP.values():
        pp.free()
    _PP.clear()


def ptable(field, bump=None):
    """the example's table: row r = (1000 + 7 r, 1 + r^2); bump: (row, col) of one element that is one more"""
    m = MOD[field]
    vals = [v for r in range(PROWS) for v in (1000 + 7 * r, 1 + r * r)]
    if bump is not None:
        vals[2 * bump[0] + bump[1]] += 1
    return vals, ts.table_array(vals, PROWS, 2, m)


@functools.lru_cache(maxsize=None)
def tables(field):
    return ptable(field), ptable(field, (2, 1))


def circuit(field, lanes=1, mode="repeat", wrong=False):
    vals, T = tables(field)[1 if wrong else 0]
    return ts.TM(T_, T, vals, mode, field, lanes=lanes)


def params(ctx, field=FIELD_FQ, lanes=1, **tune):
    key = (field, lanes, tuple(sorted(tune.items())))
    if key not in _PP:
        _PP[key] = public_params_custom(ctx, circuit(field, lanes), field=field, **tune)
    return _PP[key]


def lane_chain(field, l, wrong=False):
    vals, _ = tables(field)[1 if wrong else 0]
    return ts.minroot_chain(field, vals, PROWS, 2, 0, 1, STEPS * T_, X0 + l, 3 * l)


def z_of(field, lanes, steps, wrong=False):
    m, out = MOD[field], []
    for l in range(lanes):
        e = lane_chain(field, l, wrong)
        out += [mont_rows([v], m).tobytes() for v in e[2 * steps * T_:2 * steps * T_ + 2]]
    return out


def step_advice(field, lanes, g, wrong=False):
    """lane l's entries g t .. (g + 1) t at entry l (t + 1): flat ints"""
    out = []
    for l in range(lanes):
        out += lane_chain(field, l, wrong)[2 * g * T_:2 * ((g + 1) * T_ + 1)]
    return out


def checkpoints(field, lanes, wrong=False):
    m, out = MOD[field], []
    for l in range(lanes):
        e = lane_chain(field, l, wrong)
        out += [v for k in range(0, STEPS * T_ + 1, EVERY) for v in e[2 * k:2 * k + 2]]
    return mont_rows(out, m)


def walk_tape(field, wrong=False):
    _, T = tables(field)[1 if wrong else 0]
    return record_walk_body(ts.minroot_walk_body(field, T, 0, 1), field)


def chain_of(field, lanes=1, wrong_tape=False, wrong_cps=False):
    tape, cps = walk_tape(field, wrong_tape), checkpoints(field, lanes, wrong_cps)
    if lanes == 1:
        return CustomChain.from_checkpoints(field, tape, None, T_, EVERY, STEPS, cps)
    return CustomChain.lanes_from_checkpoints(field, tape, None, T_, EVERY, STEPS, lanes, cps)


def by_steps(pp, field, lanes, device):
    """vdf_nova_prove_step_custom step by step over host (or device) advice"""
    c, proof, m = circuit(field, lanes), None, MOD[field]
    for g in range(STEPS):
        adv = mont_rows(step_advice(field, lanes, g), m)
        c.advice = dev(adv) if device else adv
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, z_of(field, lanes, 0))
    return proof


@functools.lru_cache(maxsize=None)
def reference(ctx, field=FIELD_FQ, lanes=1):
    """the proof bytes of the plain loop over HOST advice under the default tuning; verified, compressed and verified once"""
    pp = params(ctx, field, lanes)
    proof = by_steps(pp, field, lanes, False)
    z0, zi = z_of(field, lanes, 0), z_of(field, lanes, STEPS)
    assert proof.verify(pp, STEPS, z0, zi) is True
    out = proof.serialize()
    if field == FIELD_FQ and lanes == 1:
        snark = proof.compress(pp)
        assert snark.verify(pp, STEPS, z0, zi) is True
        snark.free()
    proof.free()
    return out


def test_host_advice_device_advice_and_the_chain_give_one_proof(ctx):
    field = FIELD_FQ
    pp = params(ctx, field)
    want = reference(ctx, field)
    # the digest is the plain loop's with vdf_cs_const
    assert pp.digest() == shape_digest_custom(circuit(field, mode="loop"))[0] == shape_digest_custom(circuit(field))[0]
    proof = by_steps(pp, field, 1, True)
    assert proof.serialize() == want
    proof.free()
    chain = chain_of(field)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z_of(field, 1, 0), window_steps=2, check_steps=True)
    assert proof.verify(pp, STEPS, z_of(field, 1, 0), z_of(field, 1, STEPS)) is True
    assert proof.serialize() == want
    assert chain.memory() == (0, PROWS * 2 * 32)                   # no trace is left; the table's device copy lives with the chain
    proof.free(); chain.free()


@pytest.mark.parametrize("tune", [dict(custom_ahead=0), dict(custom_ahead=1), dict(custom_ahead=2), dict(periodic_rows=1)],
                         ids=["ahead 0", "ahead 1", "ahead 2", "periodic rows"])
def test_every_schedule_gives_the_same_bytes(ctx, tune):
    field = FIELD_FQ
    pp, chain = params(ctx, field, **tune), chain_of(field)
    if "periodic_rows" in tune:
        assert pp.periodic_rows() is None                          # rows that read a table keep the generic kernel
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z_of(field, 1, 0), window_steps=2, check_steps=True)
    assert proof.serialize() == reference(ctx, field)
    proof.free(); chain.free()


def test_two_lanes(ctx):
    field, L = FIELD_FQ, 2
    pp, want = params(ctx, field, L), reference(ctx, field, L)
    assert pp.digest() == shape_digest_custom(circuit(field, L, "loop"))[0]
    proof = by_steps(pp, field, L, True)
    assert proof.serialize() == want
    proof.free()
    chain = chain_of(field, L)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field, L), chain, z_of(field, L, 0), window_steps=2, check_steps=True)
    assert proof.serialize() == want
    proof.free(); chain.free()


def test_the_other_orientation(ctx):
    field = FIELD_FP
    pp, want, chain = params(ctx, field), reference(ctx, field), chain_of(field)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z_of(field, 1, 0), window_steps=2, check_steps=True)
    assert proof.serialize() == want
    proof.free(); chain.free()


def test_wrong_tables_are_named_and_never_fault(ctx):
    field = FIELD_FQ
    pp, z0 = params(ctx, field), z_of(field, 1, 0)
    # a walk tape whose table differs in one element: the walks of step 0 pass that row and miss their checkpoints
    chain = chain_of(field, wrong_tape=True)
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z0, window_steps=2)
    assert e.value.code == VDF_ERR_BAD_ARG and "step 0: a walk did not land on the checkpoint below it" in str(e.value)
    chain.free()
    # a round body whose table differs from the parameters'
    c = circuit(field, wrong=True)
    c.advice = mont_rows(step_advice(field, 1, 0), MOD[field])
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_step_custom(pp, None, c, z0)
    assert e.value.code == VDF_ERR_BAD_ARG and "differs from the one these parameters were made with" in str(e.value)
    # device advice made with another table (walk tape and checkpoints agree with each other, not with the circuit)
    chain = chain_of(field, wrong_tape=True, wrong_cps=True)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z0, window_steps=2)
    assert proof.verify(pp, STEPS, z0, z_of(field, 1, STEPS, wrong=True)) is False
    proof.free()
    with pytest.raises(VdfError) as e:
        NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z0, window_steps=2, check_steps=True)
    # the bumped element is c1 of row 2: y' of repetition 2 is off, and repetition 3 enforces x'^5 = x + y + c0 with that y
    assert e.value.code == VDF_ERR_BAD_ARG and "step 0:" in str(e.value) and "unsatisfied rows" in str(e.value)
    assert "repetition 3, constraint 2 of the repeat" in str(e.value)
    chain.free()
    # the context and the parameters still work
    good = chain_of(field)
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), good, z0, window_steps=2)
    assert proof.serialize() == reference(ctx, field)
    proof.free(); good.free()


# ---- g. the C example ----------------------------------------------------------------------------------------------------------
def test_the_c_example_proves_a_tabbed_chain(ctx):
    exe = os.path.join(ROOT, "examples", "prove_tabbed_chain")
    assert os.path.exists(exe), "examples/prove_tabbed_chain is built by vdf_amd/csrc/Makefile (all)"
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(T_), str(EVERY), str(STEPS), str(PROWS), str(X0)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true"
    field = FIELD_FQ
    pp, chain = params(ctx, field), chain_of(field)
    assert int(lines["digest"], 16) == pp.digest()
    proof = NovaVDFProof.prove_recursively_custom(pp, circuit(field), chain, z_of(field, 1, 0), window_steps=2, check_steps=True)
    snark = proof.compress(pp)
    assert lines["compressed proof sha256"] == hashlib.sha256(snark.serialize()).hexdigest()
    snark.free(); proof.free(); chain.free()
