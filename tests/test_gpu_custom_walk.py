"""GPU: the advice of a custom circuit's rounds rebuilt on the device by walk tapes from checkpoints (include/vdf_hip.h
vdf_round_tape_walk, kernel k_tape_walk; include/vdf_nova.h vdf_walk_body).

a. the MinRoot inverse round recorded as a walk body equals vdf_minroot_inverse_walk, trace and landings byte for byte, under the
   same strides and groups: a partial wavefront, a full one, a second and a third workgroup; both fields;
b. a body of every op on the device equals the host evaluator and a big-integer interpretation;
c. the LDS cap, the cut walk, heads, the counter's group step and expect / ok, as in tests/test_custom_walk_host.py;
d. the launcher's refusals, after which the context still works;
e. end to end: circuit F of rounds_spec proved from advice that a walk made from checkpoints -- the same proof bytes as from host
   advice; a corrupted checkpoint is reported by ok and gives a proof that does not verify, with no fault;
f. the plain-C example, as a fresh child process."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import pasta as o
from util import dev, host, mont_states, states_array
from rounds_spec import F, MOD, mont_rows
from walks_spec import (GUARD, LAYOUT, LAYOUT_ENTRIES, LAYOUT_FRONT, every_op_body, every_op_ints, expected_bytes, guarded, layout_expected,
                        minroot_body, model_walk, start_entries, tape_ints)
from vdf_amd._lib import VDF_ERR_BAD_ARG
from vdf_amd.hip import VdfError, WALK_MAX_SLOTS, WALK_MAX_WORK
from vdf_amd.minroot import EvalMode, PallasVDF, State, VestaVDF
from vdf_amd.nova import (NovaVDFProof, WalkBody, public_params_custom, record_walk_body, shape_digest_custom, walk_tape_eval, FIELD_FP,
                          FIELD_FQ)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VDF = {FIELD_FQ: PallasVDF, FIELD_FP: VestaVDF}
INV0 = 0xFEDCBA


def dguard(n_elems):
    import torch
    return torch.full((n_elems, 4), -1, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("rounds", [1, 2, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_a_minroot_inverse_tape_equals_the_inverse_walk_kernel(ctx, n, rounds, field):
    m, group, stride = MOD[field], 5, rounds + 1
    gstride = group * stride + 2                       # two entries nobody writes behind every group
    groups = (n + group - 1) // group
    tape = record_walk_body(minroot_body(field), field)
    rng = np.random.default_rng(1000 * n + rounds + field)
    xy = rng.integers(1, 2**62, size=(n, 2))
    # walk w stands on entry (w % group) * stride + rounds of group w // group; the groups' counters are 1000 apart
    rows = [(int(xy[w, 0]) ** 4, int(xy[w, 1]) ** 3, INV0 + 1000 * (w // group) + (w % group) * stride + rounds) for w in range(n)]
    states = mont_states([[v % m for v in r] for r in rows], m)
    d_states, d_entries = dev(states), dev(np.ascontiguousarray(states[:, :8]))
    want, got = dguard(2 * (groups * gstride + 1)), dguard(2 * (groups * gstride + 1))
    ctx.minroot_inverse_walk(field, d_states, n, rounds, want, walk_stride=stride, top=rounds, group=group, group_stride=gstride)
    ctx.round_tape_walk(field, tape, mont_rows([INV0], m), d_entries, n, rounds, got, walk_stride=stride, top=rounds, group=group,
                        group_stride=gstride, j_group_step=1000)
    ctx.sync()
    g, w = host(got), host(want)
    assert g.tobytes() == w.tobytes()
    assert (g.reshape(-1, 2, 4)[groups * gstride:] == np.uint64(GUARD)).all() and (g.reshape(-1, 2, 4)[0] == np.uint64(GUARD)).all()
    assert int((g.reshape(-1, 8)[:, 0] != np.uint64(GUARD)).sum()) == n * rounds   # (a canonical x never has an all-ones limb)
    assert host(d_entries).reshape(n, 8).tobytes() == np.ascontiguousarray(host(d_states).reshape(n, 12)[:, :8]).tobytes()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("rounds", [1, 5])
def test_a_body_of_every_op_on_the_device(ctx, rounds, field):
    m, n = MOD[field], 65
    tape = record_walk_body(every_op_body(field), field)
    start = start_entries(n, 3, m, np.random.default_rng(field + rounds))
    inv, kw = [m - 1], dict(walk_stride=rounds + 1, top=rounds + 1, j_base=2**64 - 3)
    n_tr = 3 * (n * (rounds + 1) + 1)
    d_entries, d_trace = dev(mont_rows(start, m)), dguard(n_tr)
    ctx.round_tape_walk(field, tape, mont_rows(inv, m), d_entries, n, rounds, d_trace, **kw)
    ctx.sync()
    entries, trace = mont_rows(start, m), guarded(n_tr)
    walk_tape_eval(field, tape, mont_rows(inv, m), entries, n, rounds, trace, **kw)
    assert host(d_entries).tobytes() == entries.tobytes() and host(d_trace).tobytes() == trace.tobytes()
    land, tr = list(start), [None] * n_tr
    model_walk(every_op_ints, m, 3, inv, land, n, rounds, tr, **kw)
    assert tape_ints(entries, m) == land and trace.tobytes() == expected_bytes(tr, m)


def wide_body(n_live, n_adv):
    """n_live values alive at once, summed into every column (live() of tests/test_custom_walk_host.py)"""
    def b(c, j, inv, nxt):
        a = [c.add(nxt[0], j)]
        for _ in range(n_live - 1):
            a.append(c.add(a[-1], a[-1]))
        s = a[0]
        for x in a[1:]:
            s = c.add(s, x)
        return [s] * n_adv
    return WalkBody(0, n_adv, b)


def test_the_lds_cap_runs_and_one_beyond_is_refused(ctx):
    """n_slots + 2 n_adv = 32 is 64 KiB of LDS: it launches and is exact; 33 is refused before a launch"""
    field, m, n, rounds, na = FIELD_FQ, o.Q, 65, 3, 5
    tape = record_walk_body(wide_body(WALK_MAX_SLOTS - 2 * na, na), field)
    assert tape.c.n_slots + 2 * na == WALK_MAX_SLOTS
    start = start_entries(n, na, m, np.random.default_rng(9))
    d_entries, entries = dev(mont_rows(start, m)), mont_rows(start, m)
    ctx.round_tape_walk(field, tape, None, d_entries, n, rounds)
    ctx.sync()
    walk_tape_eval(field, tape, None, entries, n, rounds)
    assert host(d_entries).tobytes() == entries.tobytes()
    # s = (x + j) (2^22 - 1): the body's sum of 22 doublings
    land = list(start)
    model_walk(lambda nxt, j, inv, mm: [(nxt[0] + j) * (2**22 - 1) % mm] * na, m, na, [], land, n, rounds)
    assert tape_ints(entries, m) == land
    tape.c.n_slots += 1
    with pytest.raises(VdfError):
        ctx.round_tape_walk(field, tape, None, d_entries, n, rounds)
    ctx.sync()
    assert host(d_entries).tobytes() == entries.tobytes()


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
@pytest.mark.parametrize("heads", [False, True])
def test_groups_strides_heads_the_counter_and_a_cut_walk(ctx, heads, field):
    import torch
    m = MOD[field]
    tape = record_walk_body(every_op_body(field), field)
    start, inv, want, land = layout_expected(field, heads)
    inv_m = mont_rows(inv, m)
    d_entries, d_buf = dev(mont_rows(start, m)), dguard(3 * LAYOUT_ENTRIES)
    ctx.round_tape_walk(field, tape, inv_m, d_entries, trace=d_buf[3 * LAYOUT_FRONT:], heads=heads, **LAYOUT)
    d_entries2, d_buf2 = dev(mont_rows(start, m)), dguard(3 * LAYOUT_ENTRIES)
    cut = dict(LAYOUT)
    for rounds, top, h in ((3, 5, False), (2, 2, heads)):
        cut.update(rounds=rounds, top=top)
        ctx.round_tape_walk(field, tape, inv_m, d_entries2, trace=d_buf2[3 * LAYOUT_FRONT:], heads=h, **cut)
    ctx.sync()
    assert tape_ints(host(d_entries), m) == land
    assert host(d_buf).tobytes() == expected_bytes(want, m)
    assert torch.equal(d_entries, d_entries2) and torch.equal(d_buf, d_buf2)


def test_expect_and_ok_on_the_device(ctx):
    import torch
    field, m, every, n = FIELD_FQ, o.Q, 5, 70
    tape = record_walk_body(every_op_body(field), field)
    inv = [99]
    cps = [start_entries(1, 3, m, np.random.default_rng(3))]
    for k in range(n):
        nxt = list(cps[0])
        model_walk(every_op_ints, m, 3, inv, nxt, 1, every, top=every * (n - k))
        cps.insert(0, nxt)
    wrong = [list(c) for c in cps]
    wrong[66][1] ^= 1                                  # walk 65 starts from it, walk 66 should land on it: the second workgroup
    for c, bad in ((cps, []), (wrong, [65, 66])):
        d_ok = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
        ctx.round_tape_walk(field, tape, mont_rows(inv, m), dev(mont_rows(sum(c[1:], []), m)), n, every, walk_stride=every, top=every,
                            expect=dev(mont_rows(sum(c[:-1], []), m)), ok=d_ok)
        ctx.sync()
        assert d_ok.cpu().tolist() == [0 if w in bad else 1 for w in range(n)] + [-7]


def test_the_launcher_refuses_and_the_context_goes_on(ctx):
    import torch
    field, m = FIELD_FQ, o.Q
    fresh = lambda: record_walk_body(every_op_body(field), field)
    inv = mont_rows([5], m)
    start = mont_rows(list(range(1, 13)), m)
    d_entries, d_trace, d_ok = dev(start), dguard(3 * 30), torch.zeros(4, dtype=torch.int32, device="cuda")
    good = dict(trace=d_trace, walk_stride=6, top=5)

    def refused(tape=None, entries=d_entries, rounds=5, **kw):
        args = dict(good)
        args.update(kw)
        with pytest.raises(VdfError) as e:
            ctx.round_tape_walk(field, tape or fresh(), inv, entries, 4, rounds, **args)
        assert e.value.code == VDF_ERR_BAD_ARG
    h = np.zeros((3 * 30, 4), dtype="<u8")
    refused(entries=start.copy())                      # a host pointer for entries / trace / expect / ok
    refused(trace=h)
    refused(expect=h, ok=d_ok)
    refused(expect=dev(start), ok=np.zeros(4, dtype="<i4"))
    refused(expect=dev(start))                         # expect without ok
    t = fresh()
    adv = next(i for i, x in enumerate(t.op_list()) if x[0] == 0)
    t.ops[adv].b = 0
    refused(tape=t)                                    # ADV of the entry being produced
    t = fresh()
    t.c.n_vars = 2
    refused(tape=t)                                    # n_vars != n_adv
    refused(top=3)                                     # top < rounds - 1
    refused(rounds=WALK_MAX_WORK // 3 + 1, trace=None)     # work one beyond the cap (3 products per round)
    ctx.sync()
    assert host(d_entries).tobytes() == start.tobytes() and (host(d_trace) == np.uint64(GUARD)).all() and not d_ok.cpu().any()
    # the next valid call on the same context succeeds
    ctx.round_tape_walk(field, fresh(), inv, d_entries, 4, 5, expect=dev(start), ok=d_ok, **good)
    ctx.sync()
    want, tr = start.copy(), guarded(3 * 30)
    walk_tape_eval(field, fresh(), inv, want, 4, 5, tr, walk_stride=6, top=5)
    assert host(d_entries).tobytes() == want.tobytes() and host(d_trace).tobytes() == tr.tobytes()
    ctx.round_tape_walk(field, fresh(), inv, d_entries, 0, 5)      # nothing to do
    ctx.round_tape_walk(field, fresh(), inv, d_entries, 4, 0)


# ---- end to end: circuit F (the forward MinRoot round through vdf_cs_repeat) proved from checkpoints -------------------------
@functools.lru_cache(maxsize=None)
def chain(field, t, steps, every):
    """(z0 bytes, checkpoints uint64[steps * t / every + 1, 12], the chain's last State)"""
    s0 = State.from_ints(field, 0x51DE + t, 0, 7)
    cps = VDF[field].new_with_mode(EvalMode.LTRAddChainSequential).eval_checkpoints(s0, steps * t, every)
    return (s0.x, s0.y, s0.i), states_array(cps), cps[-1]


def window_by_walks(ctx, field, t, steps, every, cps):
    """the traces of `steps` steps, (t + 1) entries each, one after the other, by ONE launch; ok per walk"""
    import torch
    per = t // every
    xy = np.ascontiguousarray(cps[:, :8])
    starts = np.concatenate([xy[g * per + 1:g * per + per + 1] for g in range(steps)])
    expect = np.concatenate([xy[g * per:g * per + per] for g in range(steps)])
    d_window, d_ok = dguard(2 * steps * (t + 1)), torch.full((steps * per,), -7, dtype=torch.int32, device="cuda")
    tape = record_walk_body(minroot_body(field), field)
    ctx.round_tape_walk(field, tape, np.ascontiguousarray(cps[0, 8:12]).reshape(1, 4), dev(starts), steps * per, every, d_window,
                        walk_stride=every, top=every, group=per, group_stride=t + 1, j_group_step=t, heads=True, expect=dev(expect), ok=d_ok)
    ctx.sync()
    return d_window, d_ok.cpu().tolist()


def prove(ctx, field, t, advice, z0):
    c = F(t, "repeat", field)
    pp = public_params_custom(ctx, c, field=field)
    proof = None
    for a in advice:
        c.advice = a
        proof = NovaVDFProof.prove_step_custom(pp, proof, c, list(z0))
    ctx.sync()
    return pp, proof


def host_traces(field, t, steps, z0):
    from util import host_trace
    s, out = State(*z0), []
    for _ in range(steps):
        s, tr = host_trace(VDF[field].new(), s, t)
        out.append(tr)
    return out


def from_checkpoints(ctx, field, t, every, steps=3, compress=False):
    z0, cps, last = chain(field, t, steps, every)
    zi = [last.x, last.y, last.i]
    d_window, ok = window_by_walks(ctx, field, t, steps, every, cps)
    assert ok == [1] * (steps * t // every)
    traces = host_traces(field, t, steps, z0)
    assert host(d_window).tobytes() == b"".join(tr.tobytes() for tr in traces)
    d_steps = d_window.view(steps, 2 * (t + 1), 4)
    pp, proof = prove(ctx, field, t, [d_steps[g] for g in range(steps)], z0)
    pp_h, proof_h = prove(ctx, field, t, traces, z0)
    assert pp.segment()[1] == 3 * t
    assert proof.serialize() == proof_h.serialize()
    assert proof.verify(pp, steps, list(z0), zi) is True
    if compress:
        snark, snark_h = proof.compress(pp), proof_h.compress(pp_h)
        assert snark.serialize() == snark_h.serialize()
        assert snark.verify(pp, steps, list(z0), zi) is True
    for p in (proof, proof_h, pp, pp_h):
        p.free()


def test_one_walk_per_step(ctx):
    from_checkpoints(ctx, FIELD_FQ, 5, 5, compress=True)


def test_a_window_of_steps_of_five_walks_each_in_one_launch(ctx):
    from_checkpoints(ctx, FIELD_FQ, 65, 13, compress=True)


def test_the_other_orientation(ctx):
    from_checkpoints(ctx, FIELD_FP, 5, 5, compress=True)


def test_a_corrupted_checkpoint_is_reported_and_its_proof_does_not_verify(ctx):
    field, t, every, steps = FIELD_FQ, 65, 13, 3
    z0, cps, last = chain(field, t, steps, every)
    wrong = cps.copy()
    wrong[7, 0] ^= np.uint64(1)                        # checkpoint 2 of step 1: walk 6 starts from it, walk 7 should land on it
    d_window, ok = window_by_walks(ctx, field, t, steps, every, wrong)
    assert ok == [0 if w in (6, 7) else 1 for w in range(15)]
    d_steps = d_window.view(steps, 2 * (t + 1), 4)
    pp, proof = prove(ctx, field, t, [d_steps[g] for g in range(steps)], z0)
    assert proof.verify(pp, steps, list(z0), [last.x, last.y, last.i]) is False
    proof.free(); pp.free()


def test_the_c_example_proves_from_checkpoints(ctx):
    exe = os.path.join(ROOT, "examples", "prove_custom_checkpoints")
    assert os.path.exists(exe), "examples/prove_custom_checkpoints is built by vdf_amd/csrc/Makefile (all)"
    t, every, steps, x0 = 65, 13, 3, 123
    # a fresh child process (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run([exe, str(t), str(every), str(steps), str(x0)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["walks ok"] == "%d of %d" % (steps * t // every, steps * t // every)
    assert lines["verify"] == "true" and lines["verify (compressed)"] == "true"
    assert int(lines["digest"], 16) == shape_digest_custom(F(t, "repeat"))[0]
    # the Python path at the same t and steps: host advice
    s0 = State.from_ints(FIELD_FQ, x0, 0, 0)
    z0 = (s0.x, s0.y, s0.i)
    pp, proof = prove(ctx, FIELD_FQ, t, host_traces(FIELD_FQ, t, steps, z0), z0)
    snark = proof.compress(pp)
    assert lines["compressed proof sha256"] == hashlib.sha256(snark.serialize()).hexdigest()
    proof.free(); pp.free()
