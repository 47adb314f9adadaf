"""What a launch of a tape, and a call over periodic rows, is refused for (vdf_amd/csrc/tape_launch.h, periodic_rules.h) as a table
like tape_rules_spec.cases(): one row for each rule at each of the seven entry points, each one mutation of a valid small call with
the status code and a substring of the message it must draw.  Both libraries read the rules from the same headers; the host test
(test_launch_rules_host.py) sends the table through the vdf_nova_*_eval restatements, the device test (test_gpu_launch_rules.py)
through the launchers and the restatements side by side.

A call is a dict of the entry point's arguments by name (ARGS, in the order of the C ABI): numpy arrays, integers, a RoundTape or a
PeriodicRows.  The valid calls: tape_rules_spec.base_tape of the mode (14 ops, 4 slots, 2 columns, 1 invariant), 3 walks of 2
rounds in 2 lanes, t = 3; the periodic rows of circuit F at t = 5.  Every output array is filled with SENTINEL words.

Rows of one entry point are in the order of its rules (Row.rule ascends); `pair` rows are the ones pairs() puts together: the later
rule's mutation first, the earlier one's on top, so both rules are broken in one call and the earlier one must be named."""
import collections
import ctypes as C
import functools

import numpy as np

import tape_rules_spec as trs
from custom_lanes_spec import wide_walk
from periodic_spec import described, operands, refusal_cases
from rounds_spec import MOD, mont_rows
from test_custom_walk_host import live
from vdf_amd._lib import VDF_ERR_BAD_ARG, VDF_ERR_BAD_LENGTH, VDF_OK
from vdf_amd.hip import FORWARD_TAPE_MAX_WORK, PERIODIC_MAX_ROWS, TAPE_MAX_LANES, WALK_MAX_SLOTS, WALK_MAX_WORK
from vdf_amd.nova import FIELD_FQ, record_forward_body, record_walk_body

FIELD = FIELD_FQ
ENTRIES = ("run", "run_lanes", "walk", "walk_lanes", "forward_walk", "rebuild_lanes", "periodic")
# (the restatement in libvdf_nova.so, the launcher in libvdf_hip.so -- which takes the context in front)
FUNCTIONS = {"run": ("vdf_nova_round_tape_eval", "vdf_round_tape_run"),
             "run_lanes": ("vdf_nova_round_tape_eval_lanes", "vdf_round_tape_run_lanes"),
             "walk": ("vdf_nova_walk_tape_eval", "vdf_round_tape_walk"),
             "walk_lanes": ("vdf_nova_walk_tape_eval_lanes", "vdf_round_tape_walk_lanes"),
             "forward_walk": ("vdf_nova_forward_tape_eval", "vdf_round_tape_forward_walk"),
             "rebuild_lanes": ("vdf_nova_forward_tape_rebuild_eval_lanes", "vdf_round_tape_rebuild_lanes"),
             "periodic": ("vdf_nova_periodic_rows_eval", "vdf_nifs_cross_term_periodic")}
ARGS = {"run": "field tape t inv advice out",
        "run_lanes": "field tape t lanes inv advice lane_stride out",
        "walk": "field tape inv entries n rounds trace walk_stride top group group_stride j_base j_group_step heads expect ok",
        "walk_lanes": "field tape lanes inv entries n rounds trace walk_stride top group group_stride j_base j_group_step heads expect ok",
        "forward_walk": "field tape inv entries n rounds checkpoints every cp_stride trace walk_stride base j_base j_walk_step",
        "rebuild_lanes": "field tape lanes inv entries n rounds trace walk_stride base group group_stride j_base j_group_step heads expect ok",
        "periodic": "field pr j_first reps seg_begin row_begin num_cols num_cons z2 az1 bz1 cz1 u1 az2 bz2 cz2 T"}
ARGS = {k: v.split() for k, v in ARGS.items()}
# the arrays a launcher reads on the host (every other array lives in device memory there)
HOST_ARRAYS = ("inv", "j_base", "u1")
MODE = {"run": trs.ROUND, "run_lanes": trs.ROUND, "walk": trs.WALK, "walk_lanes": trs.WALK, "forward_walk": trs.FORWARD,
        "rebuild_lanes": trs.FORWARD}
# field products of one round of base_tape: MUL, SCALE, MUL, SCALE; a forward tape has x^5 twice in their place, by POW (two
# squarings and a product) and by the chain (the same)
PRODUCTS = {trs.WALK: 4, trs.FORWARD: 2 + 3 + 3}
WORK = {trs.WALK: WALK_MAX_WORK, trs.FORWARD: FORWARD_TAPE_MAX_WORK}
T, LANES, N, ROUNDS, NA = 3, 2, 3, 2, trs.N_ADV
PERIODIC_T = 5

Row = collections.namedtuple("Row", "entry rule name mutate code pattern pair launcher_reaches")


def sentinel(rows, dtype="<u8"):
    if dtype == "<i4":
        return np.full(rows, -0x5A5A5A5B, dtype="<i4")
    return np.full((rows, 4), trs.SENTINEL, dtype="<u8")


def valid_call(entry):
    """a fresh valid call of the entry point: its own arrays (a periodic call shares the description, whose mutations are undone)"""
    m = MOD[FIELD]
    rng = np.random.default_rng(ENTRIES.index(entry))
    vals = lambda rows: mont_rows([int(x) for x in rng.integers(1, 2**62, size=rows)], m)
    if entry == "periodic":
        mats, pr, info = described("F", PERIODIC_T, FIELD)
        z2, a1, b1, c1, u1 = operands(FIELD, info, pr, seed=7)
        nc = info["num_cons"]
        return dict(field=FIELD, pr=pr, j_first=pr.lead, reps=PERIODIC_T - pr.lead, seg_begin=info["seg_begin"], row_begin=pr.row_begin,
                    num_cols=info["num_cols"], num_cons=nc, z2=z2, az1=a1, bz1=b1, cz1=c1, u1=u1, az2=sentinel(nc), bz2=sentinel(nc),
                    cz2=sentinel(nc), T=sentinel(nc), _undo=[])
    c = dict(field=FIELD, tape=trs.base_tape(MODE[entry], FIELD), _undo=[])
    if entry in ("run", "run_lanes"):
        lanes = 1 if entry == "run" else LANES
        c.update(t=T, inv=vals(lanes), advice=vals(lanes * (T + 1) * NA), out=sentinel(lanes * T * trs.N_ADV))
        if entry == "run_lanes":
            c.update(lanes=lanes, lane_stride=T + 1)
        return c
    c.update(inv=vals(LANES), entries=vals(N * NA), n=N, rounds=ROUNDS, trace=sentinel(12 * NA), walk_stride=3)
    if entry == "forward_walk":
        c.update(checkpoints=sentinel(12 * NA), every=1, cp_stride=3, base=0, j_base=5, j_walk_step=7)
        return c
    c.update(group=0, group_stride=0, j_base=5, j_group_step=7, heads=1, expect=vals(N * NA), ok=sentinel(N, "<i4"))
    if entry == "rebuild_lanes":
        c.update(base=0, walk_stride=2)
    else:
        c.update(top=2)
    if entry in ("walk_lanes", "rebuild_lanes"):
        c.update(lanes=LANES, group=2, group_stride=6, j_base=np.array([5, 2**64 - 1], dtype="<u8"))
    return c


def arrays(call):
    return {k: v for k, v in call.items() if isinstance(v, np.ndarray)}


def snapshot(call):
    return {k: v.tobytes() for k, v in arrays(call).items()}


def undo(call):
    while call["_undo"]:
        call["_undo"].pop()()


def host_args(entry, call, place=lambda name, array: array.ctypes.data):
    """the arguments of the C call.  place(name, array): the address an array is handed over at (the device test uploads there)"""
    out = []
    for name in ARGS[entry]:
        v = call[name]
        if isinstance(v, np.ndarray):
            v = place(name, v)
        elif name == "tape":
            v = C.addressof(v.c)
        elif name == "pr":
            v = C.addressof(v.c) if v is not None else None
        out.append(v)
    return out


# ---- the mutations ----------------------------------------------------------------------------------------------------------------
def put(**kw):
    return lambda call: call.update(kw)


def tape_op(i, **fields):
    def f(call):
        trs._set(i, **fields)(call["tape"])
    return f


def many_inv(call):
    """16 lanes of a tape with two invariants: each within its cap, the product beyond VDF_TAPE_MAX_INV"""
    call["tape"].c.n_inv = 2
    call["lanes"] = TAPE_MAX_LANES
    if call["inv"] is not None:
        call["inv"] = np.zeros((2 * (TAPE_MAX_LANES + 1), 4), dtype="<u8")
    if isinstance(call.get("j_base"), np.ndarray):
        call["j_base"] = np.zeros(TAPE_MAX_LANES + 1, dtype="<u8")


@functools.lru_cache(maxsize=None)
def _cap_tape_ops(entry):
    """the body whose tape stands exactly at VDF_WALK_MAX_SLOTS for the entry point: (record, body), n_adv = 5"""
    if entry == "walk":
        return record_walk_body, live(WALK_MAX_SLOTS - 2 * 5, n_adv=5)
    if entry == "forward_walk":
        return record_forward_body, live(WALK_MAX_SLOTS - 2 * 5, n_adv=5)
    record = record_walk_body if entry == "walk_lanes" else record_forward_body
    for n_live in range(2, WALK_MAX_SLOTS):
        if record(wide_walk(n_live, 5, 2)).c.n_slots + 2 * 5 + 2 == WALK_MAX_SLOTS:
            return record, wide_walk(n_live, 5, 2)
    raise AssertionError("no body reaches the cap")


def slot_cap(entry, beyond):
    """one walk of one round, in one lane, of a tape at the slot cap of the entry point (live values, two entries of 5 columns, in
    lanes the two invariants), or with one slot more"""
    def f(call):
        record, body = _cap_tape_ops(entry)
        tape = record(body)
        tape.c.n_slots += beyond
        tape.c.n_inv = max(tape.c.n_inv, 1)            # (an invariant no op reads, and no slot outside the lanes: a null inv stays a fault)
        call.update(tape=tape, trace=None, expect=None, ok=None, checkpoints=None, heads=0, inv=mont_rows([3, 4], MOD[FIELD]),
                    entries=mont_rows([1, 2, 3, 4, 5], MOD[FIELD]))
        if call["n"]:                                  # (a call that walks; one that only asks about the work cap stays as it is)
            call.update(n=1, rounds=1)
        if "lanes" in call:
            call["lanes"] = 1
    return f


def from_periodic(name):
    """the mutation of periodic_spec.refusal_cases by that name"""
    def f(call):
        mats, pr, info = described("F", PERIODIC_T, FIELD)
        case = {c[0]: c for c in refusal_cases(pr, info, PERIODIC_T)}[name]
        call["_undo"].append(case[1]())
        call.update(case[2])
    return f


def pr_field(name, value):
    def f(call):
        c = call["pr"].c
        old = getattr(c, name)
        setattr(c, name, value)
        call["_undo"].append(lambda: setattr(c, name, old))
    return f


def row_start(i, value):
    def f(call):
        rs = call["pr"].row_start
        old = rs[i]
        rs[i] = value
        call["_undo"].append(lambda: rs.__setitem__(i, old))
    return f


def seg_term(name, value):
    """a field of the first SEG term (the term periodic_spec's SEG cases change)"""
    def f(call):
        from vdf_amd.hip import TERM_SEG
        pr = call["pr"]
        term = next(pr.terms[i] for i in range(pr.c.n_terms) if pr.terms[i].kind == TERM_SEG)
        old = getattr(term, name)
        setattr(term, name, value(call) if callable(value) else value)
        call["_undo"].append(lambda: setattr(term, name, old))
    return f


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _rows(entry, specs):
    return [Row(entry, rule, name, mutate, code, pattern, flags.get("pair", True), flags.get("launcher_reaches", True))
            for rule, name, mutate, code, pattern, flags in specs]


def _round_rows(entry):
    lanes = entry == "run_lanes"
    A, L = VDF_ERR_BAD_ARG, VDF_ERR_BAD_LENGTH
    s = [(1, "t = 0", put(t=0), L, "t out of range", {}),
         (1, "t = 2^31", put(t=1 << 31), L, "t out of range", dict(pair=False)),
         (2, "an unknown opcode", tape_op(4, op=200), A, "tape op 4", {})]
    if lanes:
        s += [(3, "17 lanes", put(lanes=TAPE_MAX_LANES + 1), A, "lanes must be 1 .. VDF_TAPE_MAX_LANES", {}),
              (3, "no lane", put(lanes=0), A, "lanes must be 1 .. VDF_TAPE_MAX_LANES", dict(pair=False)),
              (4, "16 lanes of two invariants", many_inv, A, "lanes * n_inv > VDF_TAPE_MAX_INV (all lanes' inv travel in the kernel arguments)", {})]
    s += [(5, "null inv", put(inv=None), A, "null inv", {})]
    if lanes:
        s += [(6, "lane_stride = t", put(lane_stride=T), A, "lane_stride must be at least t + 1", {})]
    return _rows(entry, s)


def _walk_rows(entry):
    A, L = VDF_ERR_BAD_ARG, VDF_ERR_BAD_LENGTH
    lanes, forward, rebuild = entry in ("walk_lanes", "rebuild_lanes"), entry == "forward_walk", entry == "rebuild_lanes"
    mode = MODE[entry]
    most = WORK[mode] // PRODUCTS[mode]
    cap_name = "VDF_WALK_MAX_WORK" if mode == trs.WALK else "VDF_FORWARD_TAPE_MAX_WORK"
    slots = {"walk": "walk tape: n_slots + 2 * n_adv > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)",
             "walk_lanes": "walk tape in lanes: n_slots + 2 * n_adv + n_inv > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)",
             "forward_walk": "forward walk tape: n_slots + 2 * n_adv + the chains' n_tmp > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)",
             "rebuild_lanes": "rebuild tape: n_slots + 2 * n_adv + n_inv + the chains' n_tmp > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)"}[entry]
    s = [(1, "an unknown opcode", tape_op(4, op=200), A, "tape op 4", {})]
    if lanes:
        s += [(2, "17 lanes", put(lanes=TAPE_MAX_LANES + 1), A, "lanes must be 1 .. VDF_TAPE_MAX_LANES", {}),
              (2, "no lane", put(lanes=0), A, "lanes must be 1 .. VDF_TAPE_MAX_LANES", dict(pair=False)),
              (3, "16 lanes of two invariants", many_inv, A, "lanes * n_inv > VDF_TAPE_MAX_INV (all lanes' inv travel in the kernel arguments)", {})]
    s += [(4, "null inv", put(inv=None), A, "null inv", {})]
    if lanes:
        s += [(5, "null j_base", put(j_base=None), A, "null j_base", {})]
    s += [(6, "one slot beyond the cap", slot_cap(entry, 1), A, slots, {}),
          (6, "at the slot cap", slot_cap(entry, 0), VDF_OK, "", dict(pair=False)),
          (7, "far beyond the work cap", put(n=0, rounds=1 << 40), A, "rounds x products per round > %s in one call: cut the walk" % cap_name, {}),
          (7, "one round beyond the work cap", put(n=0, rounds=most + 1), A, "> " + cap_name, dict(pair=False)),
          (7, "at the work cap", put(n=0, rounds=most), VDF_OK, "", dict(pair=False))]
    if forward:
        s += [(8, "checkpoints without every", put(every=0), A, "checkpoints without `every`", {})]
    else:
        s += [(8, "expect without ok", put(ok=None), A, "expect without ok", {})]
    s += [(9, "no round", put(rounds=0), VDF_OK, "", {}),
          (9, "no walk", put(n=0), VDF_OK, "", dict(pair=False)),
          (10, "2^31 + 1 walks", put(n=(1 << 31) + 1), A if rebuild else L, "more than 2^31 walks", {}),
          # (a launcher answers a null vector by its own check of where the vectors live, ahead of this rule)
          (11, "null entries", put(entries=None), A, "null entries", dict(launcher_reaches=False))]
    if mode == trs.WALK:
        s += [(12, "top < rounds - 1", put(top=0), A, "top < rounds - 1: the walk would write below its run", {}),
              (13, "heads with top < rounds", put(top=1, heads=1), A, "heads with top < rounds: the landing would be written below the run", {})]
    if rebuild:
        s += [(12, "base + rounds > walk_stride", put(walk_stride=1), A,
               "base + rounds > walk_stride: the walk would write into the run of the walk above it", {})]
    return _rows(entry, s)


# what each case of periodic_spec.refusal_cases must be answered with, and the rule it breaks (9 .. 11: the checks of one term, in
# their order; a case on another term than the first SEG term is not paired)
_PERIODIC = {"a first repetition before the pattern's": (4, "j_first lies before the repetition the pattern was taken from", True),
             "a row range beyond num_cons": (7, "the row range ends beyond num_cons", True),
             "a bad kind": (9, ": unknown kind", True),
             "a bad constant index": (10, ": constant index out of range, or a slope on a SEG term", True),
             "a bad slope index": (10, ": constant index out of range, or a slope on a SEG term", False),
             "a fixed column at num_cols": (11, ": column beyond num_cols", False),
             "a reachable column at num_cols": (11, ": reaches a column outside [0, num_cols) in the first or the last repetition", True),
             "a reach below column 0": (11, ": reaches a column outside [0, num_cols) in the first or the last repetition", False),
             "more columns than the vectors have": (11, "num_cols", False)}


def _periodic_rows():
    A = VDF_ERR_BAD_ARG
    mats, pr, info = described("F", PERIODIC_T, FIELD)
    cases = refusal_cases(pr, info, PERIODIC_T)
    assert {c[0] for c in cases} == set(_PERIODIC)
    s = [(1, "null row_start", pr_field("row_start", None), A, "null description", {}),
         (2, "33 rows", pr_field("n_cons", PERIODIC_MAX_ROWS + 1), A, "periodic rows exceed a published cap (VDF_PERIODIC_MAX_*), or have no row or variable", {}),
         (2, "no variable", pr_field("n_vars", 0), A, "periodic rows exceed a published cap", dict(pair=False)),
         (3, "row_start begins at 1", row_start(0, 1), A, "row_start does not span the terms", {}),
         (3, "row_start descends", row_start(1, 0xFFFF), A, "row_start descends, or a row has more than VDF_PERIODIC_MAX_ROW_TERMS terms in one matrix",
          dict(pair=False)),
         (5, "no repetition", put(reps=0), VDF_OK, "", {}),
         (6, "repetitions beyond 2^32", put(reps=1 << 32), A, "more than 2^31 rows, or repetitions beyond 2^32", {}),
         (8, "no column", put(num_cols=0), A, "num_cols out of range, or seg_begin beyond it", {})]
    s += [(_PERIODIC[c[0]][0], c[0], from_periodic(c[0]), A, _PERIODIC[c[0]][1], dict(pair=_PERIODIC[c[0]][2])) for c in cases]
    return sorted(_rows("periodic", s), key=lambda r: r.rule)


@functools.lru_cache(maxsize=None)
def rows():
    out = []
    for entry in ENTRIES:
        out += _periodic_rows() if entry == "periodic" else _round_rows(entry) if entry in ("run", "run_lanes") else _walk_rows(entry)
    return tuple(out)


def pairs(launcher=False):
    """(earlier row, later row) for every two consecutive rules of an entry point.  launcher: only rules a launcher reaches"""
    out = []
    for entry in ENTRIES:
        mine = [r for r in rows() if r.entry == entry and r.pair and (r.launcher_reaches or not launcher)]
        out += [(a, b) for a, b in zip(mine, mine[1:])]
    return out


def row_id(r):
    return "%s-%d-%s" % (r.entry, r.rule, r.name.replace(" ", "_"))
