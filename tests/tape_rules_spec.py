"""The rules of a round tape (vdf_amd/csrc/tape_rules.h) as a table of tapes that break exactly one of them, each derived from
one small hand-made tape that uses every op.  Both libraries check a tape through the same header; the host test
(test_tape_rules_host.py) and the device test (test_gpu_tape_interpreter.py) send this table through their own entry points."""
import ctypes as C

import numpy as np

from rounds_spec import MOD, mont_rows
from vdf_amd.hip import RoundTape, TapeOp

ADV, INV, J, CONST, ADD, SUB, MUL, SCALE, OUT, POW, POWC = range(11)
ROUND, WALK, FORWARD = "round", "walk", "forward"
MODES = (ROUND, WALK, FORWARD)
N_SLOTS, N_ADV, N_INV, N_CONSTS = 4, 2, 1, 3
POW_NONE = 0xFF
SENTINEL = 0xA5A5A5A5A5A5A5A5          # every word of an element nothing may write (no canonical element: the top limb is too large)


def base_ops(mode):
    """(op, dst, a, b) of the valid tape of a mode: a forward tape has every op; a round tape and a descending walk tape may hold no
    POW and no POWC (a product and a scaling stand there), and load advice with the b of their mode (a round tape with both)."""
    b0, b1 = {ROUND: (0, 1), WALK: (1, 1), FORWARD: (0, 0)}[mode]
    fwd = mode == FORWARD
    return [(ADV, 0, 0, b0), (ADV, 1, 1, b1), (INV, 2, 0, 0), (J, 3, 0, 0), (ADD, 2, 2, 3), (CONST, 3, 0, 0), (SUB, 0, 0, 3), (MUL, 0, 0, 1),
            (SCALE, 1, 1, 0), (POW, 0, 0, 1) if fwd else (MUL, 0, 0, 0), (POWC, 1, 1, 2) if fwd else (SCALE, 1, 1, 0), (ADD, 0, 0, 2),
            (OUT, 0, 0, 0), (OUT, 0, 1, 1)]


def base_tape(mode, field):
    """consts: a field element, the exponent 5 as a plain integer, and the chain x -> x^5 (one step: T[0], two squarings, times T[0])"""
    t = RoundTape()
    ops = base_ops(mode)
    for i, (op, dst, a, b) in enumerate(ops):
        t.ops[i].op, t.ops[i].dst, t.ops[i].a, t.ops[i].b = op, dst, a, b
    t.consts[0] = mont_rows([7], MOD[field])[0]
    t.consts[1] = [5, 0, 0, 0]
    chain = bytes([1, 1, 0, 0, 0, 2, 0, POW_NONE]) + bytes(24)
    t.consts[2] = np.frombuffer(chain, dtype="<u8")
    t.c.ops, t.c.n_ops = C.cast(t.ops, C.POINTER(TapeOp)), len(ops)
    t.c.consts, t.c.n_consts = t.consts.ctypes.data, N_CONSTS
    t.c.n_slots, t.c.n_vars, t.c.n_cons, t.c.n_inv, t.c.n_adv = N_SLOTS, N_ADV, 0, N_INV, N_ADV
    return t


def _set(i, **fields):
    def mutate(t):
        for k, v in fields.items():
            setattr(t.ops[i], k, v)
    return mutate


def _n_vars(t):
    t.c.n_vars = 1


def _long_chain(t):
    t.consts[2, 0] = (int(t.consts[2, 0]) & ~0xFF) | 8      # 8 steps take two constants; one is left from consts[2] on


# what may stand in each field of each kind of op: one past it is malformed
_LIMITS = {ADV: dict(dst=N_SLOTS, a=N_ADV), INV: dict(dst=N_SLOTS, a=N_INV), J: dict(dst=N_SLOTS), CONST: dict(dst=N_SLOTS, a=N_CONSTS),
           ADD: dict(dst=N_SLOTS, a=N_SLOTS, b=N_SLOTS), SUB: dict(dst=N_SLOTS, a=N_SLOTS, b=N_SLOTS), MUL: dict(dst=N_SLOTS, a=N_SLOTS, b=N_SLOTS),
           SCALE: dict(dst=N_SLOTS, a=N_SLOTS, b=N_CONSTS), OUT: dict(a=N_SLOTS, b=N_ADV), POW: dict(dst=N_SLOTS, a=N_SLOTS, b=N_CONSTS),
           POWC: dict(dst=N_SLOTS, a=N_SLOTS, b=N_CONSTS)}
_NAMES = "ADV INV J CONST ADD SUB MUL SCALE OUT POW POWC".split()


def cases():
    """[(name, modes, mutate(tape), a pattern the message must hold: the op or the variable)]: the tape of each of `modes`, mutated, is refused in that mode"""
    out = [("unknown opcode", MODES, _set(4, op=200), r"tape op 4\b")]
    first = {}
    for i, (op, *_) in enumerate(base_ops(FORWARD)):
        first.setdefault(op, i)
    for op, i in sorted(first.items()):
        for f, limit in _LIMITS[op].items():
            out.append(("%s: %s one past its count" % (_NAMES[op], f), (FORWARD,) if op in (POW, POWC) else MODES, _set(i, **{f: limit}), r"tape op %d\b" % i))
    out += [("a slot read before it is written", MODES, _set(3, dst=2), r"tape op 4\b"),           # J no longer writes the slot op 4 adds
            ("a variable written twice", MODES, _set(13, b=0), r"tape op 13\b"),
            ("a variable never written", MODES, _set(13, op=J, dst=3), r"variable 1\b"),
            ("ADV with b = 2", (ROUND,), _set(0, b=2), r"tape op 0\b"),
            ("ADV of the entry a descending walk produces", (WALK,), _set(1, b=0), r"tape op 1\b"),
            ("ADV of the entry a forward walk produces", (FORWARD,), _set(1, b=1), r"tape op 1\b"),
            ("POW outside a forward tape", (ROUND, WALK), _set(9, op=POW, b=1), r"tape op 9\b"),
            ("POWC outside a forward tape", (ROUND, WALK), _set(10, op=POWC, b=2), r"tape op 10\b"),
            ("a chain that runs past n_consts", (FORWARD,), _long_chain, r"tape op 10\b"),
            ("n_vars != n_adv in a walk", (WALK, FORWARD), _n_vars, "n_vars != n_adv")]
    return out
