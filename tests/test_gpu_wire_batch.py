"""GPU: compressed proofs from wire bytes in batches -- vdf_nova_snark_deserialize_batch (every entry's points decoded by one
vdf_points_decompress per curve) and vdf_nova_verify_wire_batch (bytes in, verdicts out).  The reference for every entry is the
single call on that entry alone: its status code, and the bytes of the object it makes through both encodings; the reference for
the verdicts is vdf_nova_verify_compressed_batch over singly deserialised handles.  Then the plain-C verifier
(examples/verify_wire.c) as a fresh child process."""
import os
import subprocess

import pytest

import vdf_amd
from oracle import pasta as o
from test_gpu_nova import make
from test_gpu_verify_batch import _chain, _zi
from vdf_amd.nova import (CompressedNovaVDFProof, NovaVDFProof, CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_REFERENCE, public_params,
                          deserialize_compressed_batch, verify_compressed_batch, verify_wire_batch)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64
HEADER = 48 + 5 * 32 * 2 + 3 * 32 + 32 + 128          # magic, t, digest | three instances | T | both z_i
OK, BAD_ARG, BAD_LENGTH, NONCANONICAL = 0, 1, 2, 3


@pytest.fixture(scope="module")
def four(ctx):
    """four proofs of different chains and step counts under one parameter set: (pp, [(blob, num_steps, z0, zi)])"""
    pp, z0, circuits, _, init_ints = make(ctx, T, 2, seed=401)
    first = (NovaVDFProof.prove_recursively(pp, circuits, T, z0).compress(pp), 2, z0, _zi(init_ints))
    items = [first] + [_chain(pp, T, n, 402 + n) for n in (1, 3, 2)]
    return pp, [(s.serialize(), n, z0, zi) for s, n, z0, zi in items]


def _wire_sections(pp):
    """byte offsets into the wire encoding of the primary side's argument: the first (L, R) pair of its W opening, and its a[0]"""
    sz = pp.sizes(0)
    s = (sz["num_cons"] - 1).bit_length()
    l1 = (sz["num_vars"] - 1).bit_length() + 1
    kW = (l1 - 1) - 4
    head = HEADER + 32 * (3 * s + 4 + 2 * l1 + 1)
    return {"ipaW.L0": head, "ipaW.R0": head + 32, "ipaW.a0": head + 64 * kW}


def _put(blob, off, data):
    return blob[:off] + data + blob[off + len(data):]


def _single(pp, blob):
    """(status, flat bytes, wire bytes) of the single deserialiser for one blob"""
    try:
        s = CompressedNovaVDFProof.deserialize(pp, blob)
    except vdf_amd.VdfError as e:
        return e.code, None, None
    out = (OK, s.to_bytes(), s.serialize())
    s.free()
    return out


def _check_batch(pp, blobs):
    got = deserialize_compressed_batch(pp, blobs)
    assert len(got) == len(blobs)
    for q, ((proof, status), blob) in enumerate(zip(got, blobs)):
        want_status, flat, wire = _single(pp, blob)
        assert status == want_status, q
        assert (proof is None) == (status != OK), q
        if proof is not None:
            assert proof.to_bytes() == flat and proof.serialize() == wire == blob, q
            proof.free()
    return [status for _, status in got]


def test_every_entry_is_the_single_deserialisers_object(four):
    pp, items = four
    blobs = [it[0] for it in items]
    assert _check_batch(pp, blobs) == [OK] * 4
    assert _check_batch(pp, [blobs[2]]) == [OK]
    assert _check_batch(pp, [blobs[1], blobs[1], blobs[3]]) == [OK] * 3                    # an encoding repeated
    assert deserialize_compressed_batch(pp, []) == []


def _non_residue_x(blob, off, m):
    """the 32 bytes at `off` with x moved to the next value that is on no point of the curve (parity bit kept)"""
    v = int.from_bytes(blob[off:off + 32], "little")
    odd, x = v >> 255, v & ((1 << 255) - 1)
    while True:
        x = (x + 1) % m
        if x and pow((x * x * x + 5) % m, (m - 1) // 2, m) == m - 1:
            return (x | (odd << 255)).to_bytes(32, "little")


def _bad_blobs(ctx, pp, good):
    sect = _wire_sections(pp)
    other = public_params(ctx, T, CIRCUIT_MINROOT_BOUND)                # the same t, another circuit: another digest
    assert other.digest() != pp.digest()
    other_digest = other.digest().to_bytes(32, "little")
    other.free()
    assert good[16:48] == pp.digest().to_bytes(32, "little")
    return {
        "truncated": (good[:-1], BAD_LENGTH),
        "foreign magic": (b"VDFRSK02" + good[8:], BAD_ARG),
        "digest of another parameter set": (_put(good, 16, other_digest), BAD_ARG),
        "field element >= its modulus": (_put(good, sect["ipaW.a0"], o.Q.to_bytes(32, "little")), NONCANONICAL),
        "L_0 with x on no point": (_put(good, sect["ipaW.L0"], _non_residue_x(good, sect["ipaW.L0"], o.P)), NONCANONICAL),
        "identity with the parity bit": (_put(good, sect["ipaW.R0"], bytes(31) + b"\x80"), NONCANONICAL),
    }


def test_a_bad_entry_has_the_single_calls_status_and_leaves_its_neighbours_alone(ctx, four):
    pp, items = four
    blobs = [it[0] for it in items]
    bad = _bad_blobs(ctx, pp, blobs[1])
    for name, (blob, want) in bad.items():
        assert _single(pp, blob)[0] == want, name                       # the case is what it says
        assert _check_batch(pp, [blobs[0], blob, blobs[2]]) == [OK, want, OK], name
        assert _check_batch(pp, [blob]) == [want], name
    every = [blobs[0]] + [b for b, _ in bad.values()] + [blobs[3]]
    assert _check_batch(pp, every) == [OK] + [c for _, c in bad.values()] + [OK]
    assert _check_batch(pp, [b for b, _ in bad.values()]) == [c for _, c in bad.values()]  # nothing decodes: no point reaches the device
    assert _check_batch(pp, [b"", blobs[2], blobs[0][:40]]) == [BAD_LENGTH, OK, BAD_LENGTH]


def _reference_verdicts(pp, items):
    """what the existing pair gives: the single deserialiser per entry, the batch verifier over the handles that exist"""
    handles, live = [], []
    for q, (blob, n, z0, zi) in enumerate(items):
        try:
            handles.append((CompressedNovaVDFProof.deserialize(pp, blob), n, z0, zi))
            live.append(q)
        except vdf_amd.VdfError:
            pass
    oks = verify_compressed_batch(pp, handles)
    for h in handles:
        h[0].free()
    want = [(False, _single(pp, it[0])[0]) for it in items]
    for q, ok in zip(live, oks):
        want[q] = (ok, OK)
    return want


def test_wire_batch_verdicts_are_the_batch_verifiers(ctx, four):
    pp, items = four
    assert verify_wire_batch(pp, items) == [(True, OK)] * 4
    assert verify_wire_batch(pp, []) == []
    assert verify_wire_batch(pp, [items[2]]) == [(True, OK)]
    sect = _wire_sections(pp)
    blob1 = items[1][0]
    a0 = int.from_bytes(blob1[sect["ipaW.a0"]:sect["ipaW.a0"] + 32], "little")
    tampered = _put(blob1, sect["ipaW.a0"], ((a0 + 1) % o.Q).to_bytes(32, "little"))     # still canonical: it decodes
    assert _single(pp, tampered)[0] == OK
    undecodable = _put(items[3][0], sect["ipaW.L0"], _non_residue_x(items[3][0], sect["ipaW.L0"], o.P))
    batch = [items[0],
             (tampered,) + items[1][1:],
             (items[2][0], items[2][1], items[0][2], items[0][3]),       # entry 2's proof under entry 0's statement
             (undecodable,) + items[3][1:],
             items[3], items[2]]
    got = verify_wire_batch(pp, batch)
    assert got == [(True, OK), (False, OK), (False, OK), (False, NONCANONICAL), (True, OK), (True, OK)]
    assert got == _reference_verdicts(pp, batch)
    only_bad = [(undecodable,) + items[3][1:], (b"junk",) + items[0][1:]]
    assert verify_wire_batch(pp, only_bad) == [(False, NONCANONICAL), (False, BAD_LENGTH)] == _reference_verdicts(pp, only_bad)


def test_the_fp_orientation(ctx):
    """G1 = Vesta, G2 = Pallas: the sides' points lie on the other curves, the code is the same"""
    from test_gpu_vesta import vesta_chain, zvec
    t, n = 5, 2
    pp, z0, c, states, _, _ = vesta_chain(ctx, CIRCUIT_MINROOT_REFERENCE, t, n, seed=77)
    zi = zvec(states[0])
    snark = NovaVDFProof.prove_recursively(pp, c, t, z0).compress(pp)
    assert snark.verify(pp, n, z0, zi)
    good = snark.serialize()
    sect = _wire_sections(pp)
    bad_point = _put(good, sect["ipaW.L0"], _non_residue_x(good, sect["ipaW.L0"], o.Q))  # side 0's points are Vesta's here: over Fq
    bad_fe = _put(good, sect["ipaW.a0"], o.P.to_bytes(32, "little"))
    assert _check_batch(pp, [good, bad_point, good, bad_fe]) == [OK, NONCANONICAL, OK, NONCANONICAL]
    batch = [(good, n, z0, zi), (bad_point, n, z0, zi), (good, n, zi, z0), (good, n, z0, zi)]
    got = verify_wire_batch(pp, batch)
    assert got == [(True, OK), (False, NONCANONICAL), (False, OK), (True, OK)] == _reference_verdicts(pp, batch)
    for h in (snark, c, pp):
        h.free()


def test_the_c_verifier_as_a_child_process(tmp_path):
    """examples/prove_chain writes a proof's wire bytes; examples/verify_wire, a process that never held the prover's objects,
    verifies that file and a corrupted copy in one batch"""
    prove, verify = (os.path.join(ROOT, "examples", x) for x in ("prove_chain", "verify_wire"))
    assert os.path.exists(prove) and os.path.exists(verify), "the examples are built by vdf_amd/csrc/Makefile (all)"
    good, bad = str(tmp_path / "good.bin"), str(tmp_path / "bad.bin")
    args = ["6", "2", "123", "0"]
    # fresh child processes (never an exec of this one: the test process has initialised the GPU)
    r = subprocess.run([prove] + args + [good], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    blob = open(good, "rb").read()
    with open(bad, "wb") as f:
        f.write(_put(blob, len(blob) - 32, b"\xff" * 32))                # the last field element: not canonical
    r = subprocess.run([verify] + args + [good, bad, good], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("entry 0: ok=1 status=0 ") and lines[1].startswith("entry 1: ok=0 status=3 ")
    assert lines[2].startswith("entry 2: ok=1 status=0 ") and lines[3] == "all_ok=0"
