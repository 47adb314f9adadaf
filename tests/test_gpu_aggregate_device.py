"""GPU: the aggregate's verifier with its per-entry group arithmetic on the device (include/vdf_nova.h:
vdf_nova_aggregate_fold_instances_device, vdf_nova_verify_aggregate_device, vdf_nova_verify_aggregate_wire).  The reference for
everything is the host statement it replaces: vdf_nova_aggregate_fold_instances for the folds (byte for byte), and
vdf_nova_aggregate_deserialize + vdf_nova_verify_aggregate for the verdicts (return code, *ok, *bad_entry, decode code), on
honest and on damaged input alike.  Every proof is made at t = 2."""
import json
import os
import random
import subprocess

import pytest

import aggregate_spec as ag
from oracle import nova as nv, pasta as o, wire
from rounds_spec import F, MOD
from test_aggregate_host import golden_instance, hx, side_curve, wire_instance
from test_gpu_custom_rounds import chain as custom_chain
from test_gpu_lanes import host_lanes, lane_initials, traces_chain, zflat
from util import dev, ints
from vdf_amd.hip import VdfError
from vdf_amd.minroot import PallasVDF, VestaVDF, State, FIELD_FP, FIELD_FQ
from vdf_amd.nova import (InverseMinRootCircuit, NovaVDFProof, aggregate_fold_instances, aggregate_fold_instances_device, compress_aggregate,
                          deserialize_aggregate, public_params, public_params_custom, public_params_lanes, verify_aggregate_wire)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, BAD_LENGTH, NONCANONICAL = 0, 1, 2, 3
HEADER = 56                                            # "VDFAGG01" | t | count | digest
T = 2


def statement_bytes(arity):
    return 32 * (15 + arity)                           # r_U1 (5) | r_U2 (5) | l_u2 (3) | T2 | z_i primary (arity) | z_i secondary


def regions(K, total, arity=3):
    """name -> offset of a low byte of an element of each region of the wire: the table of tests/test_gpu_aggregate.py (which states
    it for K = 3, arity 3), with the entries it names clamped to the ones a smaller aggregate has"""
    st = statement_bytes(arity)
    tt0 = HEADER + K * st
    args = tt0 + 64 * (K - 1)
    second, last = min(1, K - 1), min(2, K - 1)
    out = {"statement: u of the second entry's running primary instance": HEADER + second * st + 64,
           "statement: comm_W of the last secondary instance": HEADER + last * st + 320,
           "statement: z_i of the first entry": HEADER + 32 * 14,
           "argument primary": args + 32 * 5, "argument secondary": total - 32 * 3}
    if K > 1:
        out["comm_TT primary"] = tt0 + 32 * min(1, K - 2)
        out["comm_TT secondary"] = tt0 + 32 * (K - 1)
    return out


def test_the_region_table_is_the_one_of_the_host_tests():
    from test_gpu_aggregate import regions as theirs
    assert regions(3, 9000) == theirs(3, 9000)


# ---- the context is left as it was found ---------------------------------------------------------------------------------------
class Untouched:
    """the context's asynchronous flag and stream before and after a call, failing calls included"""
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.before = (self.ctx.get_async(), self.ctx.stream)

    def __exit__(self, *exc):
        assert (self.ctx.get_async(), self.ctx.stream) == self.before
        return False


def outcome(call):
    """what a verifier call gives, a refusal included: ("ok", result) or ("refused", code)"""
    try:
        return ("ok", call())
    except VdfError as err:
        return ("refused", err.code)


# ---- the fold on hand-made instances -------------------------------------------------------------------------------------------
_POINTS = {}


def points(curve, n=420):
    """n distinct multiples of the generator by the oracle's addition: k G for k = k0, k0 + d, k0 + 2 d, ..."""
    if curve not in _POINTS:
        bm = o.curve_base_modulus(curve)
        rng = random.Random(0xF01D + curve)
        g = o.generator(curve)
        p = o.pt_mul(rng.randrange(1, 1 << 200), g, bm)
        d = o.pt_mul(rng.randrange(1, 1 << 200), g, bm)
        out = []
        for _ in range(n):
            out.append(p)
            p = o.pt_add(p, d, bm)
        assert len(set(out)) == n and all(o.on_curve(q, curve) for q in out[:8])
        _POINTS[curve] = out
    return _POINTS[curve]


def hand_made(primary, side, count, variant, seed):
    """count instances and count - 1 cross-term commitments without any proof.  variant: where comm_E is the identity -- "some"
    (every fifth entry; and entries 3 and count - 1 repeat entry 0, entry count - 2 repeats entry 1: equal points in one sum),
    "all" (with the identity as every second commit(TT) too) or "first" (entry 1 of the protocol only)."""
    own = primary if side == 0 else 1 - primary
    m = o.modulus(own)
    pool = points(side_curve(primary, side))
    rng = random.Random(seed)
    pick = lambda: rng.choice(pool)
    insts = []
    for k in range(count):
        if variant == "all" or (variant == "first" and k == 0) or (variant == "some" and k % 5 == 2):
            cE = (0, 0)
        else:
            cE = pick()
        insts.append(nv.Relaxed(pick(), cE, rng.randrange(m), [rng.randrange(m), rng.randrange(m)], [], []))
    if variant == "some":
        for dst, src in ((3, 0), (count - 1, 0), (count - 2, 1)):
            if 0 <= src < dst < count:
                insts[dst] = insts[src]
    tts = [(0, 0) if variant == "all" and k % 2 else pick() for k in range(count - 1)]
    return [wire_instance(U) for U in insts], [wire.compress_point(None if p == (0, 0) else p) for p in tts]


@pytest.fixture(scope="module")
def pps(ctx):
    made = {FIELD_FQ: public_params(ctx, T), FIELD_FP: public_params(ctx, T, field=FIELD_FP)}
    yield made
    for pp in made.values():
        pp.free()


@pytest.mark.parametrize("count", [1, 2, 3, 64, 65, 130])
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("primary", [FIELD_FP, FIELD_FQ], ids=["Fp", "Fq"])
def test_device_fold_equals_the_host_fold(ctx, pps, primary, side, count):
    pp = pps[primary]
    digest = pp.digest().to_bytes(32, "little")
    for variant in ("some", "all", "first"):
        inst, tts = hand_made(primary, side, count, variant, 1000 * count + 10 * side + primary)
        if variant == "some" and count >= 64:
            assert inst[3] == inst[0] == inst[count - 1] and inst[count - 2] == inst[1] and inst[2][32:64] == bytes(32)
        want = aggregate_fold_instances(primary, side, digest, inst, tts)
        with Untouched(ctx):
            got = aggregate_fold_instances_device(pp, side, inst, tts)
        assert got[1] == want[1] and len(got[1]) == count - 1, variant
        assert got[0] == want[0], variant
        if variant == "all":
            assert (got[0][32:64] == bytes(32)) == (count == 1)     # comm_E = the sum of r_k commit(TT_k) over the commit(TT) that are points


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("side", [0, 1])
def test_device_fold_equals_the_golden_file(pps, K, side):
    with open(os.path.join(ROOT, "tests", "golden", "aggregate.json")) as f:
        golden = json.load(f)
    pp = pps[FIELD_FQ]
    assert pp.digest() == hx(golden["params"])
    g = golden["aggregates"][str(K)]["sides"][side]
    inst = [wire_instance(golden_instance(j)) for j in g["instances"]]
    tts = [wire.compress_point(ag._pt(tuple(hx(v) for v in p))) for p in g["comm_TT"]]
    acc, rs = aggregate_fold_instances_device(pp, side, inst, tts)
    m = o.modulus(FIELD_FQ if side == 0 else FIELD_FP)
    assert [o.from_mont(int.from_bytes(r, "little"), m) for r in rs] == [hx(r) for r in g["r"]]
    assert acc == wire_instance(golden_instance(g["acc"]))


def test_device_fold_refusals_are_the_host_folds(ctx, pps):
    pp = pps[FIELD_FQ]
    digest = pp.digest().to_bytes(32, "little")
    inst, tts = hand_made(FIELD_FQ, 0, 3, "first", 7)
    m, bm = o.Q, o.P
    no_point = next(x for x in range(1, 99) if o.sqrt_mod((x ** 3 + 5) % bm, bm) is None).to_bytes(32, "little")
    cases = {
        "u out of range": ([inst[0], inst[1][:64] + m.to_bytes(32, "little") + inst[1][96:], inst[2]], tts),
        "X out of range": ([inst[0][:128] + b"\xff" * 32, inst[1], inst[2]], tts),
        "comm_W on no point": ([no_point + inst[0][32:], inst[1], inst[2]], tts),
        "comm_E with x out of range": ([inst[0], inst[1][:32] + bm.to_bytes(32, "little") + inst[1][64:], inst[2]], tts),
        "commit(TT) on no point": (inst, [tts[0], no_point]),
        "the identity with the parity bit": (inst, [bytes(31) + b"\x80", tts[1]]),
        "side 2": None, "no instances": ([], []), "too many": ([inst[0]] * 1025, [tts[0]] * 1024),
    }
    for name, args in cases.items():
        if name == "side 2":
            host = outcome(lambda: aggregate_fold_instances(FIELD_FQ, 2, digest, inst, tts))
            with Untouched(ctx):
                got = outcome(lambda: aggregate_fold_instances_device(pp, 2, inst, tts))
        else:
            host = outcome(lambda: aggregate_fold_instances(FIELD_FQ, 0, digest, *args))
            with Untouched(ctx):
                got = outcome(lambda: aggregate_fold_instances_device(pp, 0, *args))
        assert host[0] == "refused" and got == host, name
    assert aggregate_fold_instances_device(pp, 0, inst, tts) == aggregate_fold_instances(FIELD_FQ, 0, digest, inst, tts)


# ---- the product's aggregates --------------------------------------------------------------------------------------------------
class Made:
    """an aggregate, its bytes and its statement"""
    def __init__(self, pp, items, arity=3):
        self.pp, self.arity = pp, arity
        self.agg = compress_aggregate(pp, [it[0] for it in items])
        self.data = self.agg.serialize()
        self.stmt = ([it[1] for it in items], [list(it[2]) for it in items], [list(it[3]) for it in items])
        self.K = len(items)


class World:
    """One chain of five steps at t = 2 walked back 1 .. 5 steps from one z0: five distinct proofs under one parameter set"""
    def __init__(self, ctx, pp):
        self.pp, n = pp, 5
        initial = State.from_ints(FIELD_FQ, 0xA66, 0, 0)
        self.z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), T, n, initial)
        self.items = []
        proof = None
        for k in range(n):
            proof = NovaVDFProof.prove_step(pp, proof, circuits, k, self.z0)
            s = PallasVDF.new().eval(initial, (n - k - 1) * T) if k < n - 1 else initial
            zi = [s.x, s.y, s.i]
            assert proof.verify(pp, k + 1, self.z0, zi)
            twin = None
            for j in range(k + 1):                      # a proof object of its own for every step count
                twin = NovaVDFProof.prove_step(pp, twin, circuits, j, self.z0)
            self.items.append((twin, k + 1, self.z0, zi))
        self.made = {}

    def aggregate(self, K):
        if K not in self.made:
            self.made[K] = Made(self.pp, [self.items[k % 5] for k in range(K)])
        return self.made[K]


@pytest.fixture(scope="module")
def world(ctx, pps):
    return World(ctx, pps[FIELD_FQ])


def verdicts(ctx, made, data, stmt):
    """The three verifiers on the same bytes and statement.  Returns the host's outcome after holding the other two to it:
    the device verifier on the deserialised object, and the wire call with the deserialiser's code."""
    pp = made.pp
    try:
        agg, code = deserialize_aggregate(pp, data), OK
    except VdfError as err:
        agg, code = None, err.code
    with Untouched(ctx):
        wired = outcome(lambda: verify_aggregate_wire(pp, data, *stmt))
    if agg is None:
        assert wired == ("ok", (False, -1, code))
        return ("undecodable", code)
    host = outcome(lambda: agg.verify(pp, *stmt))
    with Untouched(ctx):
        device = outcome(lambda: agg.verify(pp, *stmt, device=True))
    assert device == host
    assert wired == (("ok", host[1] + (OK,)) if host[0] == "ok" else host)
    return host


def flipped(data, at):
    return data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]


@pytest.mark.parametrize("K", [1, 2, 3, 65])
def test_honest_aggregates_and_one_flipped_byte_per_region(ctx, world, K):
    """K = 65 names the five proofs cyclically: a proof named twice is folded twice -- equal points in the sums -- and the
    per-entry kernel crosses a wavefront (130 entries)"""
    made = world.aggregate(K)
    assert verdicts(ctx, made, made.data, made.stmt) == ("ok", (True, -1))
    assert made.agg.verify(made.pp, *made.stmt, device=True) == (True, -1)        # the prover's own object, not a decoded one
    for name, at in regions(K, len(made.data)).items():
        got = verdicts(ctx, made, flipped(made.data, at), made.stmt)
        assert got[0] == "undecodable" or got[1][0] is False, name


@pytest.mark.parametrize("K", [3, 65])
def test_wrong_statements_name_the_same_entry(ctx, world, K):
    made = world.aggregate(K)
    steps, z0, zi = made.stmt
    e = K - 2                                             # the named entry

    def changed(what):
        s, a, b = list(steps), [list(v) for v in z0], [list(v) for v in zi]
        if what == "num_steps":
            s[e] += 1
        elif what == "z0":
            a[e][0] = b[0][0]
        elif what == "zi":
            b[e][1] = a[0][0]
        elif what == "num_steps = 0":
            s[e] = 0
        return s, a, b
    for what in ("num_steps", "z0", "zi", "num_steps = 0"):
        assert verdicts(ctx, made, made.data, changed(what)) == ("ok", (False, e)), what
    sw = lambda v: [v[1], v[0]] + list(v[2:])
    assert verdicts(ctx, made, made.data, (sw(steps), sw(z0), sw(zi))) == ("ok", (False, 0))
    assert verdicts(ctx, made, made.data, (steps[:-1], z0[:-1], zi[:-1])) == ("ok", (False, -1))
    assert verdicts(ctx, made, made.data, (steps + [1], z0 + [z0[0]], zi + [zi[0]])) == ("ok", (False, -1))
    assert verdicts(ctx, made, made.data, ([], [], [])) == ("ok", (False, -1))


def test_an_asynchronous_context_stays_asynchronous(ctx, world):
    made = world.aggregate(3)
    ctx.set_async(True)
    try:
        assert verdicts(ctx, made, made.data, made.stmt) == ("ok", (True, -1))
        assert verdicts(ctx, made, made.data[:-1], made.stmt) == ("undecodable", BAD_LENGTH)
        assert ctx.get_async() is True
    finally:
        ctx.set_async(False)


def test_foreign_parameters_are_refused_alike(ctx, world, pps):
    made = world.aggregate(2)
    other = pps[FIELD_FP]
    host = outcome(lambda: made.agg.verify(other, *made.stmt))
    assert host == ("refused", BAD_ARG)
    with Untouched(ctx):
        assert outcome(lambda: made.agg.verify(other, *made.stmt, device=True)) == host
    with Untouched(ctx):
        assert verify_aggregate_wire(other, made.data, *made.stmt) == (False, -1, BAD_ARG)     # the deserialiser's code: another digest


def test_decode_codes_are_the_deserialisers(ctx, world):
    made = world.aggregate(3)
    data, pp = made.data, made.pp
    bm = o.P                                              # the primary side's commitments: Pallas, coordinates in Fp
    # an x below both moduli that is on neither curve: a canonical element wherever it stands, a point nowhere
    x = next(x for x in range(1, 999) if o.sqrt_mod((x ** 3 + 5) % o.P, o.P) is None and o.sqrt_mod((x ** 3 + 5) % o.Q, o.Q) is None)
    no_point = x.to_bytes(32, "little")
    put = lambda at: data[:at] + no_point + data[at + 32:]
    st = statement_bytes(3)
    tt0 = HEADER + 3 * st
    args = tt0 + 64 * 2
    # the first L of the primary argument: the first 32 bytes of it where those bytes are refused (elements stand in front of it)
    first_L = next(at for at in range(args, len(data), 32) if outcome(lambda: deserialize_aggregate(pp, put(at))) == ("refused", NONCANONICAL))
    assert args + 32 * 8 < first_L < len(data) - 32 * 8
    cases = {"truncated": (data[:-1], BAD_LENGTH), "shorter than the header": (data[:40], BAD_LENGTH), "one byte more": (data + b"\0", BAD_LENGTH),
             "foreign magic": (b"VDFSNK03" + data[8:], BAD_ARG), "another t": (flipped(data, 8), BAD_ARG),
             "another count": (data[:16] + (2).to_bytes(8, "little") + data[24:], BAD_LENGTH),
             "a non-canonical element": (data[:HEADER + 64] + b"\xff" * 32 + data[HEADER + 96:], NONCANONICAL),
             "no point: a statement's comm_W": (put(HEADER + st), NONCANONICAL),
             "no point: a statement's T2": (put(HEADER + 2 * st + 416), NONCANONICAL),
             "no point: commit(TT) primary": (put(tt0), NONCANONICAL), "no point: commit(TT) secondary": (put(tt0 + 96), NONCANONICAL),
             "no point: an argument's L": (put(first_L), NONCANONICAL), "no point: the last R": (put(len(data) - 32 * 17), NONCANONICAL),
             "x = the modulus in a point": (data[:HEADER] + bm.to_bytes(32, "little") + data[HEADER + 32:], NONCANONICAL)}
    for name, (bad, code) in cases.items():
        assert verdicts(ctx, made, bad, made.stmt) == ("undecodable", code), name
    # the same bytes where an element stands decode, and the aggregate does not verify
    assert verdicts(ctx, made, put(args), made.stmt)[1][0] is False


def small_world(ctx, pp, items, arity=3):
    """honest, one flipped byte per region, the first two statements swapped: all three verifiers alike"""
    made = Made(pp, items, arity)
    assert verdicts(ctx, made, made.data, made.stmt) == ("ok", (True, -1))
    for name, at in regions(made.K, len(made.data), arity).items():
        got = verdicts(ctx, made, flipped(made.data, at), made.stmt)
        assert got[0] == "undecodable" or got[1][0] is False, name
    steps, z0, zi = made.stmt
    assert verdicts(ctx, made, made.data, (steps, z0, [zi[1], zi[0]] + zi[2:])) == ("ok", (False, 0))
    pp.free()


def test_other_orientation(ctx):
    pp = public_params(ctx, T, field=FIELD_FP)
    items = []
    for x0, n in ((0x77, 1), (0x78, 2), (0x79, 1)):
        initial = State.from_ints(FIELD_FP, x0, 0, 0)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(VestaVDF.new(), T, n, initial)
        items.append((NovaVDFProof.prove_recursively(pp, circuits, T, z0), n, z0, [initial.x, initial.y, initial.i]))
    small_world(ctx, pp, items)


def test_lanes(ctx):
    L = 2
    pp = public_params_lanes(ctx, T, L)
    items = []
    for seed, n in ((61, 1), (62, 2)):
        inits, _ = lane_initials(L, seed)
        states, traces = host_lanes(T, n, inits)
        z0, lc = traces_chain(T, inits, traces)
        items.append((NovaVDFProof.prove_recursively(pp, lc, T, z0), n, z0, zflat(states[n])))
    small_world(ctx, pp, items, arity=3 * L)


def test_custom_circuit_with_a_repeat(ctx):
    c = F(T, "repeat", FIELD_FQ)
    pp = public_params_custom(ctx, c, field=FIELD_FQ)
    items, keep = [], []
    z0, traces, states = custom_chain(FIELD_FQ, T, 3)
    for n in (1, 3):
        proof = None
        for tr in traces[:n]:
            c.advice = dev(tr)
            c.advice_ints = [o.from_mont(v, MOD[FIELD_FQ]) for v in ints(tr)]
            keep.append(c.advice)
            proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
        items.append((proof, n, z0, [states[n - 1].x, states[n - 1].y, states[n - 1].i]))
    ctx.sync()
    small_world(ctx, pp, items)


def test_the_c_verifier_holds_bytes_only(world, tmp_path):
    exe = os.path.join(ROOT, "examples", "verify_aggregate")
    assert os.path.exists(exe), "examples/verify_aggregate is built by vdf_amd/csrc/Makefile (all)"
    made = world.aggregate(3)
    good, bad, stmt = tmp_path / "agg.bin", tmp_path / "bad.bin", tmp_path / "statements.txt"
    good.write_bytes(made.data)
    bad.write_bytes(flipped(made.data, regions(3, len(made.data))["argument secondary"]))
    steps, z0, zi = made.stmt
    stmt.write_text("".join("%d %s %s\n" % (steps[k], " ".join(bytes(v).hex() for v in z0[k]), " ".join(bytes(v).hex() for v in zi[k]))
                            for k in range(3)))
    # fresh child processes (never an exec of this one: the test process has initialised the GPU), each under its own time limit
    for path, want in ((good, "count=3 ok=1 bad_entry=-1 decode_code=0"), (bad, "count=3 ok=0 bad_entry=-1 decode_code=0")):
        r = subprocess.run([exe, str(T), str(path), str(stmt)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert r.stdout.strip() == want
