"""CPU tests around the device's forward walk (vdf_minroot_forward_walk / vdf_minroot_eval_batch): the boundary declares it, the
ONE statement of the two addition chains (vdf_amd/csrc/minroot_chain.h, which the host evaluator and the device kernel both
run) raises to the exponents it states next to them, and the host's four modes -- one of them that chain -- agree on the edge
inputs.  The kernel itself is tested on the GPU (tests/test_gpu_forward_walk.py)."""
import os
import re

import pytest

from oracle import pasta as o
from vdf_amd.minroot import EvalMode, PallasVDF, State, VestaVDF, FIELD_FP, FIELD_FQ, FP_RESCUE_INVALPHA, FQ_RESCUE_INVALPHA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vdf_amd", "csrc", "minroot_chain.h")


def test_prototypes_exist():
    from vdf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vdf_hip.h")).read()
    nova = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdf_nova.h")).read(), flags=re.S)
    for name, nargs in (("vdf_minroot_forward_walk", 11), ("vdf_minroot_eval_batch", 8)):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name not in nova                                      # device entry points live in vdf_hip.h only
        assert hasattr(_lib.lib, name), "libvdf_hip.so does not export " + name
        assert len(_lib.PROTOTYPES[name][1]) == nargs
    cap = int(re.search(r"#define\s+VDF_MINROOT_FORWARD_MAX_ROUNDS\s+(\d+)", hdr).group(1))
    assert cap == _lib.MINROOT_FORWARD_MAX_ROUNDS and cap >= 64
    import vdf_amd
    assert hasattr(vdf_amd.Context, "minroot_forward_walk") and hasattr(vdf_amd.Context, "minroot_eval_batch")
    assert hasattr(PallasVDF, "eval_batch")


# ---- the chain header, read as data --------------------------------------------------------------------------------

def parse_header():
    """({slot name: index}, head, {field: tail}, {field: exponent}) of minroot_chain.h; a step is (src, squarings, mul, dst) by name"""
    txt = re.sub(r"//.*", "", open(HEADER).read())
    enum = re.search(r"enum\s*:\s*uint8_t\s*\{(.*?)\};", txt, flags=re.S).group(1)
    names = {}
    for item in enum.split(","):
        k, v = [p.strip() for p in item.split("=")]
        names[k] = names[v] if v in names else int(v, 0)
    head = re.search(r"MINROOT_CHAIN_HEAD\[\]\s*=\s*\{(.*?)\};", txt, flags=re.S).group(1)
    head = [tuple(f.strip() for f in m.split(",")) for m in re.findall(r"\{([^{}]*)\}", head)]
    tails, exps = {}, {}
    for f, tag in ((FIELD_FQ, "FQ"), (FIELD_FP, "FP")):
        body = re.search(r"MINROOT_CHAIN_TAIL_%s\[\]\s*=\s*\{(.*?)\};" % tag, txt, flags=re.S).group(1)
        tails[f] = [("MR_ACC", n.strip(), m.strip(), "MR_NONE") for n, m in re.findall(r"VDF_MR_T\(([^,]*),([^)]*)\)", body)]
        limbs = re.search(r"%s_RESCUE_INVALPHA\[4\]\s*=\s*\{(.*?)\};" % tag, txt, flags=re.S).group(1)
        exps[f] = sum(int(v.strip().rstrip("ul"), 16) << (64 * k) for k, v in enumerate(limbs.split(",")))
    return names, head, tails, exps


def run_program(names, steps, slot_value, sqr, mul):
    """the interpreter of minroot_chain.h over any monoid: slot_value = the entry value of slot S1"""
    slots = {names["MR_S1"]: slot_value}
    v = slot_value
    counts = [0, 0]
    for src, n, m, dst in steps:
        if src != "MR_ACC":
            v = slots[names[src]]
        for _ in range(int(n)):
            v = sqr(v)
        counts[0] += int(n)
        if m != "MR_NONE":
            v = mul(v, slots[names[m]])
            counts[1] += 1
        if dst != "MR_NONE":
            assert names[dst] < names["MR_SLOTS"]
            slots[names[dst]] = v
    return v, counts


@pytest.mark.parametrize("field", [FIELD_FQ, FIELD_FP])
def test_chain_header_raises_to_the_exponent_it_states(field):
    names, head, tails, exps = parse_header()
    assert len(head) == 13 and names["MR_SLOTS"] == 9
    # over the exponents themselves (squaring doubles, a product adds): the program computes x^e for the header's own e ...
    e, (nsq, nmul) = run_program(names, head + tails[field], 1, lambda a: 2 * a, lambda a, b: a + b)
    assert e == exps[field]
    assert (nsq, nmul) == (253, 30 if field == FIELD_FQ else 29)
    # ... which is the reference's constant (vdf_amd/minroot.py states it from src/minroot.rs:273-285) and 1/5 mod (m - 1)
    want = FQ_RESCUE_INVALPHA if field == FIELD_FQ else FP_RESCUE_INVALPHA
    assert e == sum(l << (64 * k) for k, l in enumerate(want))
    m = o.modulus(field)
    assert 5 * e % (m - 1) == 1
    # the tails name only the eight multiplicands 1, 11, 101, 111, 1001, 1111, r4, r8
    assert {names[s[2]] for s in tails[field]} <= set(range(8))
    # and over the field itself, edge inputs included
    for x in (0, 1, m - 1, 2, o.rand_fe(5, field, m)):
        got, _ = run_program(names, head + tails[field], x, lambda a: a * a % m, lambda a, b: a * b % m)
        assert got == pow(x, e, m) and pow(got, 5, m) == x


def edge_elements(m):
    return [0, 1, m - 1, 2, m - 2, (1 << 254) - 1, (m - 1) // 2, o.rand_fe(11, 0, m)]


@pytest.mark.parametrize("V", [PallasVDF, VestaVDF])
def test_four_modes_agree_on_edge_inputs(V):
    """forward_step through the host's four modes (LTRAddChainSequential -- and VestaVDF in every mode -- runs the shared chain)
    against x^e by Python's pow, on 0, 1, m - 1 and friends"""
    f, m = V.FIELD, o.modulus(V.FIELD)
    e = sum(l << (64 * k) for k, l in enumerate(V.exponent()))
    for x in edge_elements(m):
        xb = State.from_ints(f, x, 0, 0).x
        got = {mode: V.new_with_mode(mode).forward_step(xb) for mode in EvalMode.all()}
        assert len(set(got.values())) == 1, x
        assert State(got[EvalMode.LTRAddChainSequential], xb, xb).to_ints(f)[0] == pow(x, e, m)
        assert V.inverse_step(got[EvalMode.LTRAddChainSequential]) == xb


@pytest.mark.parametrize("V", [PallasVDF, VestaVDF])
def test_rounds_with_x_plus_y_zero(V):
    """x + y = 0 (mod m): the fifth root of 0 is 0, in every mode, and the round goes on from there"""
    f, m = V.FIELD, o.modulus(V.FIELD)
    for x, y, i in ((5, m - 5, 3), (0, 0, 0), (m - 1, 1, m - 1), (0, 0, m - 1)):
        s = State.from_ints(f, x, y, i)
        outs = {mode: V.new_with_mode(mode).round(s) for mode in EvalMode.all()}
        assert len(set(outs.values())) == 1
        assert outs[EvalMode.LTRAddChainSequential].to_ints(f) == (0, (x + i) % m, (i + 1) % m)
        far = {mode: V.new_with_mode(mode).eval(s, 7) for mode in EvalMode.all()}
        assert len(set(far.values())) == 1
        want = o.minroot_eval(o.State(x, y, i), 7, f)
        assert far[EvalMode.LTRAddChainSequential].to_ints(f) == (want.x, want.y, want.i)


def test_host_sources_state_the_chains_once():
    """the tables and the exponents are in minroot_chain.h and nowhere else in the product's sources"""
    csrc = os.path.join(ROOT, "vdf_amd", "csrc")
    for dirpath, _, files in os.walk(csrc):
        if os.path.basename(dirpath) == "build" or os.sep + "build" + os.sep in dirpath + os.sep:
            continue
        for fn in files:
            if not fn.endswith((".cpp", ".hpp", ".hip", ".cuh", ".h", ".inc")) or fn == "minroot_chain.h":
                continue
            src = re.sub(r"//.*", "", open(os.path.join(dirpath, fn)).read())
            assert "0x4e9ee0c9a1" not in src.lower(), fn            # a limb both exponents share
            if "minroot_chain.h" in src:
                assert "MINROOT_CHAIN_F" in src, fn


def test_eval_farm_example_is_built():
    assert os.path.exists(os.path.join(ROOT, "examples", "eval_farm")), "examples/eval_farm is built by vdf_amd/csrc/Makefile (all)"
    assert os.path.exists(os.path.join(ROOT, "examples", "eval_farm.c"))
