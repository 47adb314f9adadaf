"""TEST INFRASTRUCTURE: the restatement of "vdf-aggregate-v1" (include/vdf_nova.h) over the oracle (oracle/nova.py,
oracle/spartan.py, oracle/wire.py: imported, never edited).  Many running proofs under one parameter set become ONE compressed
proof: per side the running instances are folded by Nova's folding scheme for two RELAXED instances, and one argument per side
is made for the two accumulators.

Everything is plain integers (canonical, not Montgomery form); a commitment is (x, y) with (0, 0) the identity, as in
oracle/nova.py."""
from __future__ import annotations

from dataclasses import dataclass, field as dc_field
from typing import List, Sequence, Tuple

from oracle import nova as nv, pasta as o, spartan, wire

MAGIC = b"VDFAGG01"
AGGREGATE_MAX = 1024


# ---- the two kernels -------------------------------------------------------------------------------------------------------
def cross_term_relaxed(az1, bz1, cz1, u1: int, az2, bz2, cz2, u2: int, m: int) -> List[int]:
    """T = Az1 o Bz2 + Az2 o Bz1 - u1 Cz2 - u2 Cz1."""
    return [(a1 * b2 + a2 * b1 - u1 * c2 - u2 * c1) % m for a1, b1, c1, a2, b2, c2 in zip(az1, bz1, cz1, az2, bz2, cz2)]


def fold_relaxed(r: int, az1, bz1, cz1, e1, az2, bz2, cz2, e2, T, m: int):
    """(Az1 + r Az2, Bz1 + r Bz2, Cz1 + r Cz2, E1 + r T + r^2 E2)."""
    r2 = r * r % m
    return (o.axpy(az1, r, az2, m), o.axpy(bz1, r, bz2, m), o.axpy(cz1, r, cz2, m),
            [(e + r * t + r2 * f) % m for e, t, f in zip(e1, T, e2)])


# ---- instances ---------------------------------------------------------------------------------------------------------------
def side_fields(field_of_primary: int, side: int) -> Tuple[int, int]:
    """(scalar modulus of the side's instances, modulus of its commitments' coordinates)."""
    own = field_of_primary if side == 0 else 1 - field_of_primary
    return o.modulus(own), o.modulus(1 - own)


def _pt(a):
    return None if tuple(a) == (0, 0) else tuple(a)


def _aff(p):
    return (0, 0) if p is None else tuple(p)


def ec_lincomb(bm: int, a, r: int, b):
    """a + r b on the curve over the field of bm."""
    return _aff(o.pt_add(_pt(a), o.pt_mul(r, _pt(b), bm), bm))


def fold_instances(field_of_primary: int, side: int, digest: bytes, insts: Sequence, comm_TT: Sequence):
    """Steps 2-3 of the protocol on instances alone.  insts: objects with comm_W, comm_E, u, X; comm_TT: len(insts) - 1 points.
    Returns (the folded instance as an nv.Relaxed without witness, the challenges)."""
    m, bm = side_fields(field_of_primary, side)
    tr = spartan.Transcript(b"aggregate")
    tr.absorb(b"count", len(insts).to_bytes(8, "little") + int(side).to_bytes(8, "little"))
    for U in insts:
        spartan._instance_bytes(tr, digest, _pt(U.comm_W), _pt(U.comm_E), U.u, U.X)
    acc = nv.Relaxed(tuple(insts[0].comm_W), tuple(insts[0].comm_E), insts[0].u, list(insts[0].X), [], [])
    rs = []
    for U, TT in zip(insts[1:], comm_TT):
        tr.absorb_pt(b"T", [_pt(TT)])
        r = tr.challenge(b"r")
        acc = fold_instance_pair(acc, U, TT, r, m, bm)
        rs.append(r)
    return acc, rs


def fold_instance_pair(a, b, TT, r: int, m: int, bm: int):
    cW = ec_lincomb(bm, a.comm_W, r, b.comm_W)
    cE = ec_lincomb(bm, ec_lincomb(bm, a.comm_E, r, TT), r * r % m, b.comm_E)
    return nv.Relaxed(cW, cE, (a.u + r * b.u) % m, [(x + r * y) % m for x, y in zip(a.X, b.X)], [], [])


# ---- witnesses: the prover's side of a fold (any shape, any commit function) ------------------------------------------------
def cross_of(shape, a, b, m: int) -> List[int]:
    az1, bz1, cz1 = o.multiply_vec(shape, list(a.W) + [a.u] + list(a.X), m)
    az2, bz2, cz2 = o.multiply_vec(shape, list(b.W) + [b.u] + list(b.X), m)
    return cross_term_relaxed(az1, bz1, cz1, a.u, az2, bz2, cz2, b.u, m)


def fold_pair(a, b, TT: Sequence[int], comm_TT, r: int, m: int, bm: int):
    """The relaxed instance-witness pair a + r b with cross term TT."""
    out = fold_instance_pair(a, b, comm_TT, r, m, bm)
    out.W = o.axpy(a.W, r, b.W, m)
    r2 = r * r % m
    out.E = [(e + r * t + r2 * f) % m for e, t, f in zip(a.E, TT, b.E)]
    return out


def fold_all(field_of_primary: int, side: int, digest: bytes, shape, commit, insts: Sequence):
    """The prover's steps 2-3: (acc with witness, [comm_TT], [r]).  commit(vector) -> point."""
    m, bm = side_fields(field_of_primary, side)
    tr = spartan.Transcript(b"aggregate")
    tr.absorb(b"count", len(insts).to_bytes(8, "little") + int(side).to_bytes(8, "little"))
    for U in insts:
        spartan._instance_bytes(tr, digest, _pt(U.comm_W), _pt(U.comm_E), U.u, U.X)
    acc, tts, rs = insts[0], [], []
    for U in insts[1:]:
        TT = cross_of(shape, acc, U, m)
        cTT = tuple(commit(TT))
        tr.absorb_pt(b"T", [_pt(cTT)])
        r = tr.challenge(b"r")
        acc = fold_pair(acc, U, TT, cTT, r, m, bm)
        tts.append(cTT)
        rs.append(r)
    return acc, tts, rs


# ---- the aggregate -----------------------------------------------------------------------------------------------------------
@dataclass
class Statement:               # what "VDFSNK03" carries in front of its arguments
    r_U1: nv.Relaxed
    r_U2: nv.Relaxed
    l_u2: nv.Fresh
    T2: tuple
    zi: List[List[int]]


@dataclass
class Aggregate:
    statements: List[Statement]
    comm_TT: List[List[tuple]]       # [side][k]
    snark1: object
    snark2: object
    trace: dict = dc_field(default_factory=dict, compare=False)     # challenges and folded instances per side (golden file)


def aggregate(pp: nv.PublicParams, proofs: Sequence[nv.RecursiveSNARK]) -> Aggregate:
    assert 1 <= len(proofs) <= AGGREGATE_MAX
    digest = int(pp.params).to_bytes(32, "little")
    sts, sides = [], ([], [])
    for s in proofs:
        f2, T2, _ = nv.nifs_fold(pp, 1, s.r[1], s.l2)
        sts.append(Statement(nv._inst_only(s.r[0]), nv._inst_only(s.r[1]), nv.Fresh(s.l2.comm_W, list(s.l2.X), []), tuple(T2),
                             [list(s.zi[0]), list(s.zi[1])]))
        sides[0].append(s.r[0])
        sides[1].append(f2)
    accs, tts, rs, args = [], [], [], []
    for side in (0, 1):
        acc, tt, r = fold_all(nv.SIDE_FIELD[0], side, digest, pp.shapes[side], lambda v, side=side: pp.commit(side, v), sides[side])
        G, U = nv.spartan_setup(pp, side)
        args.append(spartan.prove(pp.shapes[side], digest, G, U, _pt(acc.comm_W), _pt(acc.comm_E), acc.u, acc.X, acc.W, acc.E,
                                  nv.SIDE_CURVE[side]))
        accs.append(acc); tts.append(tt); rs.append(r)
    return Aggregate(sts, tts, args[0], args[1], {"r": rs, "acc": [nv._inst_only(a) for a in accs]})


def verify_aggregate(pp: nv.PublicParams, agg: Aggregate, num_steps: Sequence[int], z0: Sequence[Sequence[int]],
                     zi: Sequence[Sequence[int]]) -> Tuple[bool, int]:
    """(ok, bad_entry): the order of checks of include/vdf_nova.h."""
    K = len(agg.statements)
    if K == 0 or len(num_steps) != K:
        return False, -1
    for k in range(K):
        if num_steps[k] == 0:
            return False, k
    m2 = o.modulus(nv.SIDE_FIELD[1])
    sides = ([], [])
    for k, c in enumerate(agg.statements):
        if c.l_u2.X[0] != nv.hash_state(nv.SIDE_FIELD[0], pp.params, num_steps[k], list(z0[k]), c.zi[0], c.r_U2):
            return False, k
        if c.l_u2.X[1] != nv.hash_state(nv.SIDE_FIELD[1], pp.params, num_steps[k], [0], c.zi[1], c.r_U1):
            return False, k
        if list(c.zi[0]) != list(zi[k]) or list(c.zi[1]) != [0]:
            return False, k
        r = nv.hash_challenge(nv.SIDE_FIELD[0], pp.params, c.r_U2, c.l_u2.comm_W, c.l_u2.X, c.T2)
        f2 = nv.Relaxed(nv.ec_fold(1, c.r_U2.comm_W, r, c.l_u2.comm_W), nv.ec_fold(1, c.r_U2.comm_E, r, c.T2), (c.r_U2.u + r) % m2,
                        o.axpy(c.r_U2.X, r, c.l_u2.X, m2), [], [])
        sides[0].append(c.r_U1)
        sides[1].append(f2)
    digest = int(pp.params).to_bytes(32, "little")
    for side, pf in ((0, agg.snark1), (1, agg.snark2)):
        if len(agg.comm_TT[side]) != K - 1:
            return False, -1
        acc, _ = fold_instances(nv.SIDE_FIELD[0], side, digest, sides[side], agg.comm_TT[side])
        G, U = nv.spartan_setup(pp, side)
        if not spartan.verify(pp.shapes[side], digest, G, U, _pt(acc.comm_W), _pt(acc.comm_E), acc.u, acc.X, pf, nv.SIDE_CURVE[side]):
            return False, -1
    return True, -1


# ---- "VDFAGG01" --------------------------------------------------------------------------------------------------------------
def encode_statement(c: Statement) -> bytes:
    out = wire.encode_instance(c.r_U1, True) + wire.encode_instance(c.r_U2, True) + wire.encode_instance(c.l_u2, False)
    out += wire.compress_point(_pt(c.T2))
    return out + b"".join(wire.fe(v) for v in c.zi[0]) + b"".join(wire.fe(v) for v in c.zi[1])


def encode(t: int, params: int, agg: Aggregate) -> bytes:
    out = MAGIC + int(t).to_bytes(8, "little") + len(agg.statements).to_bytes(8, "little") + int(params).to_bytes(32, "little")
    out += b"".join(encode_statement(c) for c in agg.statements)
    for side in (0, 1):
        out += b"".join(wire.compress_point(_pt(p)) for p in agg.comm_TT[side])
    return out + wire.encode_argument(agg.snark1, wire.compress_point) + wire.encode_argument(agg.snark2, wire.compress_point)


IPA_STOP = 16


def _argument_dims(shape):
    M, NW, Z = spartan._layout(shape)
    rounds = lambda n: max(0, (n.bit_length() - 1) - 4)
    return M.bit_length() - 1, Z.bit_length() - 1, (rounds(NW), min(NW, IPA_STOP)), (rounds(M), min(M, IPA_STOP))


def argument_size(shape) -> int:
    s, l1, (kw, aw), (ke, ae) = _argument_dims(shape)
    return 32 * (3 * s + 4 + 2 * l1 + 1 + aw + ae) + 64 * (kw + ke)


class _Reader:
    def __init__(self, data: bytes):
        self.d, self.i = data, 0

    def take(self, n: int) -> bytes:
        if self.i + n > len(self.d):
            raise ValueError("truncated")
        self.i += n
        return self.d[self.i - n:self.i]

    def fe(self, m: int) -> int:
        v = int.from_bytes(self.take(32), "little")
        if v >= m:
            raise ValueError("element out of range")
        return v

    def pt(self, curve: int):
        return wire.decompress_point(self.take(32), curve)


def _decode_argument(rd: _Reader, shape, side: int):
    m, curve = o.modulus(nv.SIDE_FIELD[side]), nv.SIDE_CURVE[side]
    s, l1, dw, de = _argument_dims(shape)
    outer = [[rd.fe(m) for _ in range(3)] for _ in range(s)]
    claims = tuple(rd.fe(m) for _ in range(4))
    inner = [[rd.fe(m) for _ in range(2)] for _ in range(l1)]
    w = rd.fe(m)
    ipas = []
    for k, a in (dw, de):
        L, R = [], []
        for _ in range(k):
            L.append(rd.pt(curve)); R.append(rd.pt(curve))
        ipas.append(spartan.IpaProof(L, R, [rd.fe(m) for _ in range(a)]))
    return spartan.SpartanProof(outer, claims, inner, w, ipas[0], ipas[1])


def decode(data: bytes, t: int, params: int, arity: int, shapes) -> Aggregate:
    """ValueError unless `data` is exactly an encoding under (t, params, shapes)."""
    rd = _Reader(data)
    if rd.take(8) != MAGIC:
        raise ValueError("magic")
    if int.from_bytes(rd.take(8), "little") != t:
        raise ValueError("t")
    K = int.from_bytes(rd.take(8), "little")
    if int.from_bytes(rd.take(32), "little") != params:
        raise ValueError("digest")
    per = 32 * (5 + 5 + 3 + 1 + arity + 1)
    if not 1 <= K <= AGGREGATE_MAX or len(data) != 56 + K * per + 64 * (K - 1) + argument_size(shapes[0]) + argument_size(shapes[1]):
        raise ValueError("length")
    m = [o.modulus(nv.SIDE_FIELD[s]) for s in (0, 1)]
    cv = nv.SIDE_CURVE

    def inst(side, relaxed):
        cW = _aff(rd.pt(cv[side]))
        if relaxed:
            cE, u = _aff(rd.pt(cv[side])), rd.fe(m[side])
        X = [rd.fe(m[side]) for _ in range(2)]
        return nv.Relaxed(cW, cE, u, X, [], []) if relaxed else nv.Fresh(cW, X, [])

    sts = []
    for _ in range(K):
        U1, U2, l2 = inst(0, True), inst(1, True), inst(1, False)
        T2 = _aff(rd.pt(cv[1]))
        sts.append(Statement(U1, U2, l2, T2, [[rd.fe(m[0]) for _ in range(arity)], [rd.fe(m[1])]]))
    tts = [[_aff(rd.pt(cv[side])) for _ in range(K - 1)] for side in (0, 1)]
    a1 = _decode_argument(rd, shapes[0], 0)
    a2 = _decode_argument(rd, shapes[1], 1)
    assert rd.i == len(data)
    return Aggregate(sts, tts, a1, a2)


# ---- a hand-made tiny R1CS for the folding tests -----------------------------------------------------------------------------
def tiny_shape(m: int, seed: int = 1, num_cons: int = 8, num_vars: int = 6):
    """8 constraints over z = (W[6], u, X[2]): row i multiplies two random sparse combinations; C selects what makes a random
    assignment satisfiable is the caller's business (relaxed_from_assignment computes E)."""
    import random
    rng = random.Random(seed)
    cols = num_vars + 3
    mat = lambda: [(r, c, rng.randrange(1, m)) for r in range(num_cons) for c in rng.sample(range(cols), 2)]
    return o.R1CSShape(num_cons, num_vars, 2, mat(), mat(), mat())


def random_relaxed(shape, m: int, rng, commit):
    """A satisfiable relaxed pair: random W, u, X, and E = Az o Bz - u Cz."""
    W = [rng.randrange(m) for _ in range(shape.num_vars)]
    u = rng.randrange(1, m)
    X = [rng.randrange(m) for _ in range(2)]
    az, bz, cz = o.multiply_vec(shape, W + [u] + X, m)
    E = [(a * b - u * c) % m for a, b, c in zip(az, bz, cz)]
    return nv.Relaxed(tuple(commit(W)), tuple(commit(E)), u, X, W, E)
