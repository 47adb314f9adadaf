"""GPU: many running proofs aggregated into one compressed proof (vdf_nova_compress_aggregate / vdf_nova_verify_aggregate,
"vdf-aggregate-v1" in include/vdf_nova.h).

The scenario of tests/golden/make_aggregate.py -- the reference's circuit at t = 2, one chain walked back 1, 2 and 3 steps from a
fixed z0 -- is proved by the product, and the aggregates of the first K = 1, 2, 3 proofs must have the oracle's bytes (length and
SHA-256 committed in tests/golden/aggregate.json).  Then what the header promises around that: K = 1 is vdf_nova_compress, the
proofs go on proving, a proof may be named twice, every region of the wire is bound, the per-entry checks name their entry, and
the refusals.  One make -> serialize -> deserialize -> verify each for the other orientation, a lanes parameter set and a custom
circuit with a vdf_cs_repeat; the C example as a child process."""
import hashlib
import json
import os
import subprocess

import pytest

from oracle import pasta as o
from rounds_spec import F, MOD
from test_gpu_custom_rounds import chain as custom_chain
from test_gpu_lanes import host_lanes, lane_initials, traces_chain, zflat
from util import dev, ints
from vdf_amd.hip import VdfError
from vdf_amd.minroot import PallasVDF, VestaVDF, State, FIELD_FP, FIELD_FQ
from vdf_amd.nova import (AGGREGATE_MAX, InverseMinRootCircuit, NovaVDFProof, compress_aggregate, deserialize_aggregate, public_params,
                          public_params_custom, public_params_lanes)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_LENGTH, NONCANONICAL = 1, 2, 3
HEADER, STATEMENT = 56, 32 * 18                      # "VDFAGG01" | t | count | digest; a statement at arity 3


def state_bytes(ints):
    s = State.from_ints(FIELD_FQ, *ints)
    return [s.x, s.y, s.i]


class World:
    """The golden scenario on the device: pp, the proofs of 1, 2 and 3 steps (and untouched twins), their statements."""

    def __init__(self, ctx):
        with open(os.path.join(ROOT, "tests", "golden", "aggregate.json")) as f:
            self.golden = json.load(f)
        g = self.golden
        self.t, self.n = g["t"], len(g["entries"])
        self.pp = public_params(ctx, self.t)
        assert self.pp.digest() == int(g["params"], 16)
        initial = State.from_ints(FIELD_FQ, int(g["x0"], 16), 0, 0)
        self.z0, self.circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), self.t, self.n, initial)
        assert b"".join(self.z0) == b"".join(state_bytes([int(v, 16) for v in g["entries"][0]["z0"]]))
        self.steps = [e["num_steps"] for e in g["entries"]]
        self.zi = [state_bytes([int(v, 16) for v in e["zi"]]) for e in g["entries"]]
        self.proofs = [self.prove(n) for n in self.steps]
        self.twins = [self.prove(n) for n in self.steps]
        for p, n, zi in zip(self.proofs, self.steps, self.zi):
            assert p.verify(self.pp, n, self.z0, zi)
        self.aggs = {K: compress_aggregate(self.pp, self.proofs[:K]) for K in (1, 2, 3)}
        self.bytes = {K: a.serialize() for K, a in self.aggs.items()}

    def prove(self, n, proof=None, first=0):
        for k in range(first, n):
            proof = NovaVDFProof.prove_step(self.pp, proof, self.circuits, k, self.z0)
        return proof

    def statement(self, K):
        return self.steps[:K], [self.z0] * K, self.zi[:K]


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.pp.free()                                          # with its proofs and aggregates: the compression queues go back to the pool


def refusal(call):
    """(code, message) of the VdfError `call` raises.  The exception is not kept: a frame that holds one holds, through its
    traceback, every parameter set of the frames below it until the cycle collector runs."""
    try:
        call()
    except VdfError as err:
        return err.code, str(err)
    pytest.fail("the call was not refused")


@pytest.mark.parametrize("K", [1, 2, 3])
def test_aggregate_bytes_are_the_oracles(world, K):
    want = world.golden["aggregates"][str(K)]
    data = world.bytes[K]
    assert world.aggs[K].count == K
    assert (len(data), hashlib.sha256(data).hexdigest()) == (want["len"], want["sha256"])
    assert world.aggs[K].verify(world.pp, *world.statement(K)) == (True, -1)
    back = deserialize_aggregate(world.pp, data)
    assert back.serialize() == data and back.count == K
    assert back.verify(world.pp, *world.statement(K)) == (True, -1)


def test_one_proof_aggregated_is_its_compression(world):
    """K = 1 folds nothing: statement and both arguments are those of vdf_nova_compress, byte for byte (the wire's 32-byte points
    encode the flat encoding's 64-byte points one to one)."""
    snark = world.prove(1).compress(world.pp).serialize()
    assert world.bytes[1][HEADER:] == snark[48:]
    assert len(world.bytes[1]) == len(snark) + 8


def test_the_proofs_go_on_proving_to_the_same_bytes(world):
    """After three aggregations the 1-step and the 2-step proof take one more step: the bytes of their untouched twins."""
    for j in (0, 1):
        assert world.proofs[j].serialize() == world.twins[j].serialize()
        a = world.prove(world.steps[j] + 1, world.proofs[j], first=world.steps[j])
        b = world.prove(world.steps[j] + 1, world.twins[j], first=world.steps[j])
        assert a.serialize() == b.serialize()
        assert a.verify(world.pp, world.steps[j] + 1, world.z0, world.zi[j + 1])
    # (proofs[0] and proofs[1] have moved on: the tests below make their own)


@pytest.fixture(scope="module")
def trio(world):
    """three fresh proofs of 1, 2 and 3 steps, their aggregate and its bytes"""
    proofs = [world.prove(n) for n in world.steps]
    agg = compress_aggregate(world.pp, proofs)
    data = agg.serialize()
    assert data == world.bytes[3]
    return proofs, agg, data


def test_the_same_proof_twice(world, trio):
    proofs, _, _ = trio
    agg = compress_aggregate(world.pp, [proofs[1], proofs[2], proofs[1]])
    steps, z0, zi = world.statement(3)
    pick = lambda v: [v[1], v[2], v[1]]
    assert agg.verify(world.pp, pick(steps), pick(z0), pick(zi)) == (True, -1)
    assert deserialize_aggregate(world.pp, agg.serialize()).verify(world.pp, pick(steps), pick(z0), pick(zi)) == (True, -1)


def regions(K, total):
    """name -> offset of a low byte of an element of each region of the wire"""
    tt0 = HEADER + K * STATEMENT
    args = tt0 + 64 * (K - 1)
    return {"statement: u of the second entry's running primary instance": HEADER + STATEMENT + 64,
            "statement: comm_W of the last secondary instance": HEADER + 2 * STATEMENT + 320,
            "statement: z_i of the first entry": HEADER + 32 * 14,
            "comm_TT primary": tt0 + 32, "comm_TT secondary": tt0 + 32 * (K - 1),
            "argument primary": args + 32 * 5, "argument secondary": total - 32 * 3}


@pytest.mark.parametrize("region", sorted(regions(3, 0)))
def test_one_flipped_byte_anywhere_is_refused(world, trio, region):
    """A statement, a cross-term commitment of either side, either argument: the aggregate does not verify, or the bytes do not
    decode (VDF_ERR_NONCANONICAL: a flipped x is on no point, or an element left its range)."""
    _, _, data = trio
    at = regions(3, len(data))[region]
    bad = data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]
    made = []
    try:
        made.append(deserialize_aggregate(world.pp, bad))
    except VdfError as err:
        assert err.code == NONCANONICAL, region
    for agg in made:
        assert agg.verify(world.pp, *world.statement(3))[0] is False, region


def test_decode_errors_have_their_codes(world, trio):
    _, _, data = trio
    for bad, code in ((b"VDFSNK03" + data[8:], BAD_ARG), (data[:8] + bytes([data[8] ^ 1]) + data[9:], BAD_ARG),
                      (data[:24] + bytes([data[24] ^ 1]) + data[25:], BAD_ARG), (data[:-1], BAD_LENGTH), (data + b"\0", BAD_LENGTH),
                      (data[:16] + (2).to_bytes(8, "little") + data[24:], BAD_LENGTH), (data[:16] + bytes(8) + data[24:], BAD_LENGTH),
                      (data[:16] + b"\xff" * 8 + data[24:], BAD_LENGTH), (data[:40], BAD_LENGTH),
                      (data[:HEADER + 64] + b"\xff" * 32 + data[HEADER + 96:], NONCANONICAL)):
        assert refusal(lambda: deserialize_aggregate(world.pp, bad))[0] == code


@pytest.mark.parametrize("what", ["num_steps", "z0", "zi"])
def test_a_wrong_statement_names_its_entry(world, trio, what):
    _, agg, _ = trio
    steps, z0, zi = world.statement(3)
    steps, z0, zi = list(steps), [list(v) for v in z0], [list(v) for v in zi]
    if what == "num_steps":
        steps[1] += 1
    elif what == "z0":
        z0[1][0] = zi[0][0]
    else:
        zi[1][1] = z0[0][0]
    assert agg.verify(world.pp, steps, z0, zi) == (False, 1)


def test_statements_swapped_or_miscounted(world, trio):
    _, agg, _ = trio
    steps, z0, zi = world.statement(3)
    sw = lambda v: [v[1], v[0], v[2]]
    assert agg.verify(world.pp, sw(steps), sw(z0), sw(zi)) == (False, 0)
    assert agg.verify(world.pp, steps[:2], z0[:2], zi[:2]) == (False, -1)
    assert agg.verify(world.pp, steps + [1], z0 + [z0[0]], zi + [zi[0]]) == (False, -1)
    assert agg.verify(world.pp, [0] + steps[1:], z0, zi) == (False, 0)
    assert agg.verify(world.pp, steps, z0, zi) == (True, -1)
    # the entries in another order are another aggregate: its own statement order verifies, the first one's does not
    proofs, _, _ = trio
    other = compress_aggregate(world.pp, sw(proofs))
    assert other.verify(world.pp, sw(steps), sw(z0), sw(zi)) == (True, -1)
    assert other.verify(world.pp, steps, z0, zi)[0] is False


def test_compress_aggregate_refusals(ctx, world, trio):
    proofs, _, data = trio
    pp2 = public_params(ctx, world.t + 1)
    z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), world.t + 1, 1, State.from_ints(FIELD_FQ, 5, 0, 0))
    other = NovaVDFProof.prove_step(pp2, None, circuits, 0, z0)
    for args, code, text in (([], BAD_ARG, "count"), ([proofs[0]] * (AGGREGATE_MAX + 1), BAD_ARG, "count"),
                             ([proofs[0], None, proofs[1]], BAD_ARG, "entry 1"), ([proofs[0], proofs[1], other], BAD_ARG, "entry 2")):
        got = refusal(lambda: compress_aggregate(world.pp, args))
        assert got[0] == code and text in got[1], got
    foreign = compress_aggregate(pp2, [other])                          # an aggregate of other parameters
    assert refusal(lambda: foreign.verify(world.pp, [1], [z0], [z0]))[0] == BAD_ARG
    # nothing was disturbed
    assert compress_aggregate(world.pp, proofs).serialize() == data
    pp2.free()


# ---- one make -> serialize -> deserialize -> verify each ----------------------------------------------------------------------
def round_trip(pp, items):
    """items: [(proof, num_steps, z0, zi)]"""
    agg = compress_aggregate(pp, [it[0] for it in items])
    back = deserialize_aggregate(pp, agg.serialize())
    stmt = ([it[1] for it in items], [it[2] for it in items], [it[3] for it in items])
    assert back.verify(pp, *stmt) == (True, -1)
    wrong = (stmt[0], stmt[1], [stmt[2][1], stmt[2][0]])
    assert back.verify(pp, *wrong) == (False, 0)
    pp.free()


def test_smoke_other_orientation(ctx):
    t = 4
    pp = public_params(ctx, t, field=FIELD_FP)
    items = []
    for x0, n in ((0x77, 1), (0x78, 2)):
        initial = State.from_ints(FIELD_FP, x0, 0, 0)
        z0, circuits = InverseMinRootCircuit.eval_and_make_circuits(VestaVDF.new(), t, n, initial)
        items.append((NovaVDFProof.prove_recursively(pp, circuits, t, z0), n, z0, [initial.x, initial.y, initial.i]))
    round_trip(pp, items)


def test_smoke_lanes(ctx):
    L, t = 2, 4
    pp = public_params_lanes(ctx, t, L)
    items = []
    for seed, n in ((61, 1), (62, 2)):
        inits, _ = lane_initials(L, seed)
        states, traces = host_lanes(t, n, inits)
        z0, lc = traces_chain(t, inits, traces)
        items.append((NovaVDFProof.prove_recursively(pp, lc, t, z0), n, z0, zflat(states[n])))
    round_trip(pp, items)


def test_smoke_custom_circuit_with_a_repeat(ctx):
    t = 4
    c = F(t, "repeat", FIELD_FQ)
    pp = public_params_custom(ctx, c, field=FIELD_FQ)
    assert pp.segment()[1] == 3 * t
    items, keep = [], []
    z0, traces, states = custom_chain(FIELD_FQ, t, 3)
    for n in (1, 3):
        proof = None
        for tr in traces[:n]:
            c.advice = dev(tr)
            c.advice_ints = [o.from_mont(v, MOD[FIELD_FQ]) for v in ints(tr)]
            keep.append(c.advice)
            proof = NovaVDFProof.prove_step_custom(pp, proof, c, z0)
        items.append((proof, n, z0, [states[n - 1].x, states[n - 1].y, states[n - 1].i]))
    ctx.sync()
    round_trip(pp, items)


def test_the_c_example_aggregates_three_chains(tmp_path):
    exe = os.path.join(ROOT, "examples", "aggregate_proofs")
    assert os.path.exists(exe), "examples/aggregate_proofs is built by vdf_amd/csrc/Makefile (all)"
    out = tmp_path / "agg.bin"
    # a fresh child process (never an exec of this one: the test process has initialised the GPU), under its own time limit
    r = subprocess.run([exe, "3", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    data = out.read_bytes()
    assert lines["verified from the bytes"].startswith("true") and lines["sha256"] == hashlib.sha256(data).hexdigest()
    assert data[:8] == b"VDFAGG01" and int.from_bytes(data[16:24], "little") == 3
