"""CPU tests of "vdf-aggregate-v1" (include/vdf_nova.h): the restatement (tests/aggregate_spec.py) on a hand-made R1CS, the
product's host-only verifier fold vdf_nova_aggregate_fold_instances against it and against tests/golden/aggregate.json, the
wire format's round trip in the restatement, and the entry points' presence in headers, libraries and the Rust file.  No device
call is made."""
import copy
import json
import os
import random
import re

import pytest

import aggregate_spec as ag
from oracle import nova as nv, pasta as o, spartan, wire

import vdf_amd.nova as vn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, FQ = o.FIELD_FP, o.FIELD_FQ
NONCANONICAL, BAD_ARG = 3, 1


@pytest.fixture(scope="module")
def golden_agg():
    with open(os.path.join(ROOT, "tests", "golden", "aggregate.json")) as f:
        return json.load(f)


# ---- the folding scheme for two relaxed instances, on 8 constraints ----------------------------------------------------------
class Tiny:
    """A shape of 8 constraints over `field`, Pedersen generators on the curve whose scalars that field is, as side 0 of the
    orientation field_of_primary = field."""

    def __init__(self, field):
        self.field, self.m = field, o.modulus(field)
        self.curve = o.CURVE_PALLAS if field == FQ else o.CURVE_VESTA
        self.bm = o.curve_base_modulus(self.curve)
        self.shape = ag.tiny_shape(self.m, seed=11 + field)
        self.G = o.synthetic_bases(self.curve, 77, 8)
        self.digest = bytes(range(32))

    def commit(self, v):
        return ag._aff(o.msm_naive(list(v), self.G[:len(v)], self.curve))

    def sat(self, U):
        return (o.is_sat_relaxed(self.shape, U.W, U.E, U.u, U.X, self.m) and self.commit(U.W) == tuple(U.comm_W)
                and self.commit(U.E) == tuple(U.comm_E))

    def pair(self, seed):
        rng = random.Random(seed)
        return [ag.random_relaxed(self.shape, self.m, rng, self.commit) for _ in range(2)]


@pytest.fixture(scope="module", params=[FP, FQ], ids=["Fp", "Fq"])
def tiny(request):
    return Tiny(request.param)


def test_two_relaxed_instances_fold_to_a_satisfiable_one(tiny):
    a, b = tiny.pair(1)
    assert tiny.sat(a) and tiny.sat(b) and any(a.E) and any(b.E) and a.u != 1 and b.u != 1
    acc, tts, rs = ag.fold_all(tiny.field, 0, tiny.digest, tiny.shape, tiny.commit, [a, b])
    assert tiny.sat(acc) and len(tts) == len(rs) == 1 and 0 < rs[0] < 1 << 128
    # the verifier reaches the same instance from instances and the cross-term commitment alone
    inst, rv = ag.fold_instances(tiny.field, 0, tiny.digest, [a, b], tts)
    assert rv == rs and (inst.comm_W, inst.comm_E, inst.u, inst.X) == (acc.comm_W, acc.comm_E, acc.u, acc.X)


@pytest.mark.parametrize("what", ["TT", "r", "E2", "u2"])
def test_a_single_change_breaks_the_fold(tiny, what):
    """The fold is satisfiable only with the cross term of exactly these two instances, E folded with r^2 E2 for the very r that
    folded W, and the second instance's own u in both the cross term and the fold."""
    a, b = tiny.pair(2)
    m, bm = tiny.m, tiny.bm
    TT = ag.cross_of(tiny.shape, a, b, m)
    r = 0x1234567890ABCDEF1234567890ABCDEF
    good = ag.fold_pair(a, b, TT, tiny.commit(TT), r, m, bm)
    assert tiny.sat(good)
    if what == "TT":
        TT = list(TT); TT[3] = (TT[3] + 1) % m
        bad = ag.fold_pair(a, b, TT, tiny.commit(TT), r, m, bm)
    elif what == "r":                                     # E folded with another challenge than W, u and X
        bad = copy.deepcopy(good)
        other = ag.fold_pair(a, b, TT, tiny.commit(TT), r + 1, m, bm)
        bad.E, bad.comm_E = other.E, other.comm_E
    elif what == "E2":                                    # the r^2 E2 term left out: the strict-instance fold applied to a relaxed one
        bad = copy.deepcopy(good)
        bad.E = [(e + r * t) % m for e, t in zip(a.E, TT)]
        bad.comm_E = tiny.commit(bad.E)
    else:                                                 # u2 taken for 1, as vdf_cross_term does
        TT = o.cross_term(*o.multiply_vec(tiny.shape, a.W + [a.u] + a.X, m), *o.multiply_vec(tiny.shape, b.W + [b.u] + b.X, m), a.u, m)
        bad = ag.fold_pair(a, b, TT, tiny.commit(TT), r, m, bm)
    assert tiny.commit(bad.W) == tuple(bad.comm_W) and tiny.commit(bad.E) == tuple(bad.comm_E)
    assert not o.is_sat_relaxed(tiny.shape, bad.W, bad.E, bad.u, bad.X, m)


def test_four_sequential_folds_stay_satisfiable(tiny):
    insts = tiny.pair(3) + tiny.pair(4) + tiny.pair(5)[:1]
    acc, tts, rs = ag.fold_all(tiny.field, 0, tiny.digest, tiny.shape, tiny.commit, insts)
    assert len(rs) == 4 and len(set(rs)) == 4 and tiny.sat(acc)
    inst, rv = ag.fold_instances(tiny.field, 0, tiny.digest, insts, tts)
    assert rv == rs and (inst.comm_W, inst.comm_E, inst.u, inst.X) == (acc.comm_W, acc.comm_E, acc.u, acc.X)


def test_the_kernels_restatement_reduces_to_the_strict_fold():
    m = o.Q
    rng = random.Random(9)
    v = [[rng.randrange(m) for _ in range(5)] for _ in range(8)]
    assert ag.cross_term_relaxed(v[0], v[1], v[2], 7, v[3], v[4], v[5], 1, m) == o.cross_term(v[0], v[1], v[2], v[3], v[4], v[5], 7, m)
    got = ag.fold_relaxed(3, v[0], v[1], v[2], v[6], v[3], v[4], v[5], [0] * 5, v[7], m)
    assert got == tuple(o.axpy(x, 3, y, m) for x, y in ((v[0], v[3]), (v[1], v[4]), (v[2], v[5]), (v[6], v[7])))


# ---- vdf_nova_aggregate_fold_instances -----------------------------------------------------------------------------------------
def wire_instance(U) -> bytes:
    return wire.encode_instance(U, True)


def from_wire(data: bytes, curve: int):
    f = lambda i: int.from_bytes(data[32 * i:32 * i + 32], "little")
    return (ag._aff(wire.decompress_point(data[:32], curve)), ag._aff(wire.decompress_point(data[32:64], curve)), f(2), [f(3), f(4)])


def product_fold(field_of_primary, side, digest, insts, tts):
    m, _ = ag.side_fields(field_of_primary, side)
    acc, rs = vn.aggregate_fold_instances(field_of_primary, side, digest, [wire_instance(U) for U in insts],
                                          [wire.compress_point(ag._pt(p)) for p in tts])
    return acc, [o.from_mont(int.from_bytes(r, "little"), m) for r in rs]


def side_curve(field_of_primary, side):
    own = field_of_primary if side == 0 else 1 - field_of_primary
    return o.CURVE_PALLAS if own == FQ else o.CURVE_VESTA


def random_instances(field_of_primary, side, count, seed, identity_E=()):
    """Instances with commitments that are points of the side's curve (no witness: the verifier's fold never sees one)"""
    m, bm = ag.side_fields(field_of_primary, side)
    g = o.generator(side_curve(field_of_primary, side))
    rng = random.Random(seed)
    pt = lambda: ag._aff(o.pt_mul(rng.randrange(1, m), g, bm))
    insts = [nv.Relaxed(pt(), (0, 0) if k in identity_E else pt(), rng.randrange(m), [rng.randrange(m), rng.randrange(m)], [], [])
             for k in range(count)]
    return insts, [pt() for _ in range(count - 1)]


@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("primary", [FP, FQ], ids=["Fp", "Fq"])
def test_product_fold_equals_the_restatement(primary, side, count):
    """Either orientation, either side, counts 1 .. 3, the identity as comm_E of the first and of the last instance."""
    digest = bytes(range(100, 132))
    insts, tts = random_instances(primary, side, count, 40 + count, identity_E=(0, count - 1))
    want, rs = ag.fold_instances(primary, side, digest, insts, tts)
    acc, got_r = product_fold(primary, side, digest, insts, tts)
    assert got_r == rs and all(r < 1 << 128 for r in rs)
    assert acc == wire_instance(want)
    assert from_wire(acc, side_curve(primary, side)) == (want.comm_W, want.comm_E, want.u, want.X)


def test_identity_everywhere_folds_to_the_identity():
    insts, tts = random_instances(FQ, 0, 2, 50, identity_E=(0, 1))
    acc, _ = product_fold(FQ, 0, bytes(32), insts, [(0, 0)])
    assert acc[32:64] == bytes(32)                       # comm_E = O + r O + r^2 O
    want, _ = ag.fold_instances(FQ, 0, bytes(32), insts, [(0, 0)])
    assert acc == wire_instance(want)


def hx(v):
    return int(v, 16)


def golden_instance(j):
    return nv.Relaxed(tuple(hx(v) for v in j["comm_W"]), tuple(hx(v) for v in j["comm_E"]), hx(j["u"]), [hx(v) for v in j["X"]], [], [])


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("side", [0, 1])
def test_product_fold_equals_the_golden_file(golden_agg, K, side):
    """The oracle's scenario (tests/golden/make_aggregate.py): the committed challenges and folded instances per side.  Entry 1 is
    the 1-step proof: on side 0 its comm_E is the identity."""
    g = golden_agg["aggregates"][str(K)]["sides"][side]
    digest = hx(golden_agg["params"]).to_bytes(32, "little")
    insts = [golden_instance(j) for j in g["instances"]]
    if side == 0:
        assert insts[0].comm_E == (0, 0)
    tts = [tuple(hx(v) for v in p) for p in g["comm_TT"]]
    acc, rs = product_fold(FQ, side, digest, insts, tts)
    assert rs == [hx(r) for r in g["r"]] and len(rs) == K - 1
    assert acc == wire_instance(golden_instance(g["acc"]))
    want, rs2 = ag.fold_instances(FQ, side, digest, insts, tts)
    assert rs2 == rs and wire_instance(want) == acc


def test_a_flipped_bit_in_any_absorbed_field_changes_every_later_challenge():
    """Every instance is absorbed before the first challenge: a bit of ANY instance (the last one included), of the digest, of the
    count or of the side moves every challenge; a bit of a cross-term commitment moves its own and every later one."""
    digest = bytes(range(32))
    insts, tts = random_instances(FQ, 0, 4, 60)
    _, base = product_fold(FQ, 0, digest, insts, tts)
    assert len(set(base)) == 3

    def moved(insts2=insts, tts2=tts, digest2=digest, side=0):
        _, rs = product_fold(FQ, side, digest2, insts2, tts2)
        return [a != b for a, b in zip(base, rs)]

    m, bm = ag.side_fields(FQ, 0)
    g = o.generator(o.CURVE_PALLAS)
    for k in range(4):
        for fieldname in ("comm_W", "comm_E", "u", "X0", "X1"):
            c = copy.deepcopy(insts)
            if fieldname in ("comm_W", "comm_E"):
                setattr(c[k], fieldname, ag._aff(o.pt_add(ag._pt(getattr(c[k], fieldname)), g, bm)))
            elif fieldname == "u":
                c[k].u ^= 1
            else:
                c[k].X[int(fieldname[1])] ^= 1
            assert moved(insts2=c) == [True] * 3, (k, fieldname)
    assert moved(digest2=bytes([1]) + digest[1:]) == [True] * 3
    for k in range(3):
        t2 = list(tts)
        t2[k] = ag._aff(o.pt_add(ag._pt(t2[k]), g, bm))
        assert moved(tts2=t2) == [False] * k + [True] * (3 - k), k
    # the count and the side are absorbed: a prefix of the same instances, or the same bytes on the other side, draw other challenges
    _, fewer = product_fold(FQ, 0, digest, insts[:3], tts[:2])
    assert all(a != b for a, b in zip(base, fewer))
    spec_side0 = ag.fold_instances(FQ, 0, digest, insts, tts)[1]
    tr = spartan.Transcript(b"aggregate")
    tr.absorb(b"count", (4).to_bytes(8, "little") + (1).to_bytes(8, "little"))
    for U in insts:
        spartan._instance_bytes(tr, digest, ag._pt(U.comm_W), ag._pt(U.comm_E), U.u, U.X)
    tr.absorb_pt(b"T", [ag._pt(tts[0])])
    assert spec_side0 == base and tr.challenge(b"r") != base[0]


def test_fold_instances_refusals():
    insts, tts = random_instances(FQ, 0, 2, 70)
    w = [wire_instance(U) for U in insts]
    t = [wire.compress_point(ag._pt(p)) for p in tts]
    good = vn.aggregate_fold_instances(FQ, 0, bytes(32), w, t)
    assert len(good[0]) == 160
    off = next(x for x in range(1, 100) if o.sqrt_mod((x ** 3 + 5) % o.P, o.P) is None)     # an x that is on no point of Pallas
    for args, code in (((7, 0, bytes(32), w, t), BAD_ARG), ((FQ, 2, bytes(32), w, t), BAD_ARG), ((FQ, 0, bytes(32), [], []), BAD_ARG),
                       ((FQ, 0, bytes(32), [w[0], w[1][:64] + b"\xff" * 32 + w[1][96:]], t), NONCANONICAL),        # u >= m
                       ((FQ, 0, bytes(32), [bytes([off]) + bytes(31) + w[0][32:], w[1]], t), NONCANONICAL),
                       ((FQ, 0, bytes(32), w, [bytes(31) + b"\x80"]), NONCANONICAL)):                             # the identity has one encoding
        with pytest.raises(vn.VdfError) as e:
            vn.aggregate_fold_instances(*args)
        assert e.value.code == code, args[:2]


# ---- the wire format in the restatement ------------------------------------------------------------------------------------------
def fake_argument(shape, side, rng):
    m, bm = o.modulus(nv.SIDE_FIELD[side]), o.curve_base_modulus(nv.SIDE_CURVE[side])
    g = o.generator(nv.SIDE_CURVE[side])
    s, l1, dw, de = ag._argument_dims(shape)
    fe = lambda: rng.randrange(m)
    pt = lambda: o.pt_mul(rng.randrange(1, 1 << 64), g, bm)
    ipa = lambda d: spartan.IpaProof([pt() for _ in range(d[0])], [pt() for _ in range(d[0])], [fe() for _ in range(d[1])])
    return spartan.SpartanProof([[fe() for _ in range(3)] for _ in range(s)], tuple(fe() for _ in range(4)),
                                [[fe() for _ in range(2)] for _ in range(l1)], fe(), ipa(dw), ipa(de))


@pytest.mark.parametrize("K", [1, 3])
def test_wire_round_trip_in_the_restatement(K):
    """decode(encode(x)) == x, the identity as comm_E and as a cross-term commitment included; the layout's length; truncation,
    a foreign magic, another t or digest and an element out of range are refused."""
    rng = random.Random(80 + K)
    shapes = [o.R1CSShape(40, 70, 2, [], [], []), o.R1CSShape(20, 9, 2, [], [], [])]
    sts = []
    for k in range(K):
        (U1,), _ = random_instances(FQ, 0, 1, 90 + k, identity_E=(0,) if k == 0 else ())
        (U2,), _ = random_instances(FQ, 1, 1, 95 + k)
        (l2,), (T2,) = random_instances(FQ, 1, 1, 97 + k)[0], random_instances(FQ, 1, 2, 99 + k)[1]
        sts.append(ag.Statement(U1, U2, nv.Fresh(l2.comm_W, l2.X, []), T2, [[rng.randrange(o.Q) for _ in range(3)], [0]]))
    tts = [random_instances(FQ, side, K, 110 + side)[1] for side in (0, 1)]
    if K > 1:
        tts[0][0] = (0, 0)
    x = ag.Aggregate(sts, tts, fake_argument(shapes[0], 0, rng), fake_argument(shapes[1], 1, rng))
    data = ag.encode(5, 0xABCDEF, x)
    assert data[:8] == b"VDFAGG01" and len(data) == 56 + K * 32 * 18 + 64 * (K - 1) + ag.argument_size(shapes[0]) + ag.argument_size(shapes[1])
    assert ag.decode(data, 5, 0xABCDEF, 3, shapes) == x
    assert ag.encode(5, 0xABCDEF, ag.decode(data, 5, 0xABCDEF, 3, shapes)) == data
    for bad in (data[:-1], data + b"\0", b"VDFSNK03" + data[8:]):
        with pytest.raises(ValueError):
            ag.decode(bad, 5, 0xABCDEF, 3, shapes)
    for args in ((6, 0xABCDEF), (5, 0xABCDEE)):
        with pytest.raises(ValueError):
            ag.decode(data, *args, 3, shapes)
    u_at = 56 + 64                                       # u of the first statement's r_U1
    with pytest.raises(ValueError):
        ag.decode(data[:u_at] + b"\xff" * 32 + data[u_at + 32:], 5, 0xABCDEF, 3, shapes)


def test_golden_lengths_follow_the_layout(golden_agg):
    """Each further proof costs a statement (18 elements at arity 3) and two points: 640 bytes."""
    lens = [golden_agg["aggregates"][str(K)]["len"] for K in (1, 2, 3)]
    assert lens[1] - lens[0] == lens[2] - lens[1] == 32 * 18 + 64
    assert [e["num_steps"] for e in golden_agg["entries"]] == [1, 2, 3]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
NOVA_ENTRY_POINTS = ("vdf_nova_compress_aggregate", "vdf_nova_verify_aggregate", "vdf_nova_aggregate_free", "vdf_nova_aggregate_count",
                     "vdf_nova_aggregate_serialized_size", "vdf_nova_aggregate_serialize", "vdf_nova_aggregate_deserialize",
                     "vdf_nova_aggregate_fold_instances")
HIP_ENTRY_POINTS = ("vdf_cross_term_relaxed", "vdf_fold_relaxed")


def test_every_entry_point_is_in_header_library_and_rust_file():
    import ctypes
    from vdf_amd import _lib
    rust = open(os.path.join(ROOT, "bindings", "rust", "vdf-hip-sys", "src", "lib.rs")).read()
    for names, header, lib in ((NOVA_ENTRY_POINTS, "vdf_nova.h", vn.nova_lib), (HIP_ENTRY_POINTS, "vdf_hip.h", _lib.lib)):
        text = open(os.path.join(ROOT, "include", header)).read()
        for name in names:
            assert re.search(r"\b%s\s*\(" % name, text), (name, header)
            assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
            assert re.search(r"pub fn %s\(" % name, rust), name
    assert "VDF_NOVA_AGGREGATE_MAX 1024" in open(os.path.join(ROOT, "include", "vdf_nova.h")).read() and vn.AGGREGATE_MAX == ag.AGGREGATE_MAX == 1024
    assert "pub struct VdfWireInstance" in rust and "pub struct VdfAggregate" in rust
