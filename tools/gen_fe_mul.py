#!/usr/bin/env python3
"""Emit vdf_amd/csrc/fe_mul_gfx950.inc, fe_sqr_gfx950.inc and fe_mul2_gfx950.inc: the bodies of the gfx950 Montgomery
products (product scanning, 96-bit column accumulator) with ONE asm statement per column -- and fe_{mul,sqr,mul2}_t31_gfx950.inc,
the same columns for multiplicands whose limb 7 is at most 2^31 (every value of the lazy domain: fe.cuh), where that bound lets
more carry adds of columns 7..14 go.

hipcc pads every boundary between two consecutive inline-asm statements with s_nop and zero-initialises `hi` with a
v_mov per column; generating the columns (each with its exact number of products and reduction terms, and the first
carry-add WRITING hi instead of accumulating into it) removes both.  Column k accumulates a[i]*b[k-i] and q[k-1]*m1,
q[k-2]*m2, q[k-3]*m3, q[k-7]*m7 (m0 = 1 is handled by the shift step, m4..m6 are zero).

A product costs v_mad_u64_u32 (64-bit accumulate, carry to VCC) and, only where that carry can be set, v_addc_co_u32
(carry into hi).  Every operand name has an upper bound (BOUNDS below: 32-bit limbs and quotient digits, the modulus limbs
at their maximum over both fields), and the generator tracks an exact integer upper bound of the accumulator through the
whole scan.  Within a column the terms are ordered by ascending bound and the carry add is emitted only from the first
term at which bound(acc) + bound(term) reaches 2^64: before it the 64-bit accumulator holds the true sum, so VCC is clear
and hi (not yet written) stands for zero.  The first emitted carry add of a column writes hi; a column with none hands
the shift step a constant zero.  The sum of a column does not depend on the order of its terms and hi counts exactly the
overflows that happen, so the result is bit for bit what the schedule with every carry add gives; that schedule is kept
in each file under VDF_FE_CARRY_ALL for A/B builds.

  gen_fe_mul.py            write the six files
  gen_fe_mul.py --check    regenerate them in memory and fail on any difference from the committed files

schedule() and model() expose the same column lists as a pure-integer model of the emitted schedule (64-bit wrapping
accumulator, hi incremented only where a carry add is emitted, an assertion at every dropped one): tests/test_fe_scan_model.py."""
import os
import sys

B32 = (1 << 32) - 1
MODULI = {"fp": 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
          "fq": 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001}


def limbs(v, n=8):
    return [(v >> (32 * i)) & B32 for i in range(n)]


for _m in MODULI.values():
    _l = limbs(_m)
    assert _l[0] == 1 and _l[4] == _l[5] == _l[6] == 0 and _l[7] == 1 << 30 and (-pow(_m, -1, 1 << 32)) % (1 << 32) == B32
# the modulus limbs the reduction multiplies by, at their maximum over both fields
M_MAX = {"m%d" % i: max(limbs(m)[i] for m in MODULI.values()) for i in (1, 2, 3, 7)}
RED = ((1, "m1"), (2, "m2"), (3, "m3"), (7, "m7"))
BODIES = ("mul", "sqr", "mul2")

MAD = "v_mad_u64_u32 %[acc], vcc, %[{x}], %[{y}], %[acc]"
MAD0 = "v_mad_u64_u32 %[acc], vcc, %[{x}], %[{y}], 0"
ADDC_FIRST = "v_addc_co_u32_e64 %[hi], vcc, 0, 0, vcc"
ADDC = "v_addc_co_u32_e32 %[hi], vcc, 0, %[hi], vcc"


TOP31 = 1 << 31          # the bounded-top bodies: limb 7 of every multiplicand is at most this (a lazy value is below 2^255 + 2^224)


def bound(body, name, top31=False):
    """upper bound of an operand: limbs of A, B, C, D, the squaring's shifted limbs and the quotient digits are 32-bit words
    (nothing is assumed about the operands beyond 256 bits), d8 of the squaring is the carry of 2a, the modulus limbs are constants.
    top31: limb 7 of every multiplicand is at most 2^31 -- a7, b7, c7, d7 of the products, a7 alone of the squaring (d7, s7 and d8
    are limbs of 2a, which that does not bound)"""
    if name in M_MAX:
        return M_MAX[name]
    if body == "sqr" and name == "d8":
        return 1
    if top31 and name in (("a7",) if body == "sqr" else ("a7", "b7", "c7", "d7")):
        return TOP31
    return B32


def operand(body, name):
    """asm input constraint and C expression of an operand name"""
    if name[0] == "m":
        return '"s"(%s)' % name.upper()
    if name[0] == "q":
        return '"v"(q[%s])' % name[1:]
    src = {"a": "A", "s": "S", "d": "D"} if body == "sqr" else {"a": "A", "b": "B", "c": "Cc", "d": "Dd"}
    return '"v"(%s[%s])' % (src[name[0]], name[1:])


def sqr_products(k):
    """Column k of a^2 = sum_i a_i * E_i * B^(2i), E_i = [a_i, S_(i+1), D_(i+2), ..., D_8]: S_j = (a_j << 1) mod 2^32 and D = the limbs
    of 2a (D_8 = its carry), so that E_i = a_i + 2 (a div B^(i+1)) B -- 43 products instead of 64."""
    out = []
    for i in range(8):
        j = k - i
        if j == i:
            out.append(("a%d" % i, "a%d" % i))
        elif j == i + 1 and i <= 6:
            out.append(("a%d" % i, "s%d" % j))
        elif i + 2 <= j <= 8 and i <= 6:
            out.append(("a%d" % i, "d%d" % j))
    return out


assert sum(len(sqr_products(k)) for k in range(15)) == 43


def column_terms(body, k):
    """(products of the first statement, products of the second statement, reduction terms) of column k"""
    if body == "sqr":
        first, second = sqr_products(k), []
    else:
        idx = [(i, k - i) for i in range(8) if 0 <= k - i <= 7]
        first = [("a%d" % i, "b%d" % j) for i, j in idx]
        second = [("c%d" % i, "d%d" % j) for i, j in idx] if body == "mul2" else []
    reds = [("q%d" % (k - d), name) for d, name in RED if 0 <= k - d <= 7]
    return first, second, reds


class Term:
    def __init__(self, x, y, bound, second):
        self.x, self.y, self.bound, self.second = x, y, bound, second
        self.carry = None        # None: carry add dropped; "first": the hi-writing form; "acc": accumulates into hi

    def __repr__(self):
        return "%s*%s" % (self.x, self.y)


class Column:
    """terms in emission order; entry = bound of acc when the column starts, total = bound of (hi : acc) when it ends"""
    def __init__(self, k, terms, entry, total):
        self.k, self.terms, self.entry, self.total = k, terms, entry, total
        self.has_hi = any(t.carry for t in terms)


def schedule(body, carry_all=False, top31=False):
    """the 15 columns of a body.  carry_all: the order and the carry adds of the schedule before the bound argument (every
    product followed by its carry add); otherwise ascending bounds and only the carry adds that can see a carry.
    top31: the bounded-top body (bound())"""
    assert not (carry_all and top31)
    cols, entry = [], 0
    for k in range(15):
        first, second, reds = column_terms(body, k)
        terms = [Term(x, y, bound(body, x, top31) * bound(body, y, top31), False) for x, y in first]
        terms += [Term(x, y, bound(body, x, top31) * bound(body, y, top31), True) for x, y in second]
        rterms = [Term(x, y, bound(body, x) * bound(body, y), bool(second)) for x, y in reds]
        if carry_all:
            terms += rterms
        else:
            # the reduction terms belong to the first statement (30 asm operands allow it); the second product's terms stay
            # behind the first's (they share its bounds; with a bounded top limb the ascending order holds within each statement)
            for t in rterms:
                t.second = False
            terms = sorted(rterms + terms, key=lambda t: (t.second, t.bound))
            assert [t.second for t in terms] == sorted(t.second for t in terms)
        running, emitting = entry, carry_all
        for t in terms:
            running += t.bound
            if not emitting and running >= 1 << 64:
                emitting = True
            if emitting:
                t.carry = "acc"
        for t in terms:
            if t.carry:
                t.carry = "first"
                break
        assert running < 1 << 96
        cols.append(Column(k, terms, entry, running))
        # (lo, mid, hi) -> (mid, hi) + [lo != 0] in a reducing column (the quotient digit times m0 = 1 clears lo and carries)
        entry = (running >> 32) + (1 if k < 8 else 0)
    # what is left after column 14 is the ninth word: the callers' operand ranges keep it zero (fe.cuh), the scan does not need it
    return cols


def dropped(body, top31=False):
    return sum(1 for c in schedule(body, top31=top31) for t in c.terms if not t.carry)


def emit_statement(body, col, terms, first_stmt, hi_live):
    lines, ins = [], {}
    for t in terms:
        zero = col.k == 0 and first_stmt and t is terms[0]
        lines.append((MAD0 if zero else MAD).format(x=t.x, y=t.y))
        for n in (t.x, t.y):
            ins[n] = operand(body, n)
        if t.carry:
            lines.append(ADDC_FIRST if t.carry == "first" else ADDC)
    outs = '[acc] "=&v"(acc)' if (col.k == 0 and first_stmt) else '[acc] "+v"(acc)'
    if any(t.carry for t in terms):
        outs += ', [hi] "%s"(hi)' % ("+v" if hi_live else "=&v")
    inputs = ", ".join("[%s] %s" % (n, v) for n, v in ins.items())
    return '  asm("%s"\n      : %s\n      : %s\n      : "vcc");' % ("\\n\\t".join(lines), outs, inputs)


def emit_body(body, carry_all, top31=False):
    out = ["  uint32_t q[8];\n  uint64_t acc;\n  uint32_t hi;"]
    if not carry_all:
        out.append('  static_assert(%s, "the carry adds were dropped for modulus limbs within these bounds (tools/gen_fe_mul.py)");'
                   % " && ".join("%s <= 0x%08xu" % (n.upper(), v) for n, v in M_MAX.items()))
    if top31:
        out.append('  static_assert(TOP7 <= 0x%08xu, "the carry adds were dropped for multiplicands whose limb 7 is within this bound (tools/gen_fe_mul.py)");' % TOP31)
    for col in schedule(body, carry_all, top31):
        k = col.k
        if carry_all:
            out.append("  // ---- column %d ----" % k)
        else:
            gone = [t for t in col.terms if not t.carry]
            out.append("  // ---- column %d: acc <= 0x%x on entry, (hi : acc) <= 0x%x after %d terms; %s ----"
                       % (k, col.entry, col.total, len(col.terms),
                          "no carry add after %s (running bound 0x%x < 2^64)" % (", ".join(map(repr, gone)), col.entry + sum(t.bound for t in gone))
                          if gone else "every carry add kept"))
        one = [t for t in col.terms if not t.second]
        two = [t for t in col.terms if t.second]
        out.append(emit_statement(body, col, one, True, False))
        if two:
            out.append(emit_statement(body, col, two, False, any(t.carry for t in one)))
        if k < 8 and carry_all:
            out.append("  q[%d] = 0u - (uint32_t)acc;\n  %s;" % (k, "col_shift_q(acc, hi)" if col.has_hi else "col_shift_q0(acc)"))
        elif k < 8:
            out.append("  q[%d] = %s;" % (k, "col_shift_qf(acc, hi)" if col.has_hi else "col_shift_qf0(acc)"))
        elif col.has_hi:
            out.append("  r[%d] = (uint32_t)acc;\n  acc = (acc >> 32) | ((uint64_t)hi << 32);" % (k - 8))
        else:
            out.append("  r[%d] = (uint32_t)acc;\n  acc = acc >> 32;" % (k - 8))
    out.append("  r[7] = (uint32_t)acc;")
    return out


HEADERS = {
    # a*b (fe_mul_inl, fe_mul_lazy)
    "mul": ["// GENERATED by tools/gen_fe_mul.py -- do not edit.  Included inside fe_mul_inl (fe.cuh).",
            "// Inputs: const uint32_t* A, * B; constexpr M1, M2, M3, M7.  Outputs: uint32_t r[8] (< 2m, before the",
            "// final conditional subtraction)."],
    # a*a (fe_sqr_lazy, fe.cuh): 43 products + 32 reduction products; the same integer (a^2 + q m) / 2^256 as the general product's
    "sqr": ["// GENERATED by tools/gen_fe_mul.py -- do not edit.  Included inside fe_sqr_lazy (fe.cuh).",
            "// Inputs: const uint32_t* A (below 2^256), S[j] = A[j] << 1 (j = 1..7), D[j] = limb j of 2A (j = 2..8); constexpr M1, M2, M3, M7.",
            "// Outputs: uint32_t r[8] = (A*A + q*m) / 2^256 -- bit for bit what fe_mul_gfx950.inc gives for B = A."],
    # a*b + c*d with ONE shared reduction (fe_mul2_lazy, fe.cuh): 128 products + 32 reduction products instead of 2 x 96;
    # inputs below 2m + eps give a result below 3m + eps (bound argument at fe_mul2_lazy).  clang allows 30 operands per asm
    # statement: the second product's terms get a statement of their own, accumulating into the (acc, hi) the first one left
    "mul2": ["// GENERATED by tools/gen_fe_mul.py -- do not edit.  Included inside fe_mul2_lazy (fe.cuh).",
             "// Inputs: const uint32_t* A, * B, * Cc, * Dd; constexpr M1, M2, M3, M7.  Outputs: uint32_t r[8] =",
             "// (A*B + Cc*Dd + q*m) / 2^256, below 3m + eps for inputs below 2m + eps."],
}


T31_ENTRY = {"mul": "fe_mul_lazy_t31", "sqr": "fe_sqr_lazy_t31", "mul2": "fe_mul2_lazy_t31"}


def render_t31(body):
    """the bounded-top body: the same columns with limb 7 of every multiplicand at most 2^31 (fe.cuh: the lazy domain's values)"""
    mads = sum(len(c.terms) for c in schedule(body, top31=True))
    n = dropped(body, top31=True)
    out = ["// GENERATED by tools/gen_fe_mul.py -- do not edit.  Included inside %s (fe.cuh)." % T31_ENTRY[body]]
    out += HEADERS[body][1:]
    out.append("// PRECONDITION: limb 7 of %s is at most 0x%08x; constexpr TOP7 is the bound the including function vouches for."
               % ("A" if body == "sqr" else "every multiplicand (%s)" % ", ".join(["A", "B", "Cc", "Dd"][:2 if body == "mul" else 4]), TOP31))
    out.append("// %d v_mad_u64_u32, %d v_addc_co_u32: %d carry adds dropped (%d without that precondition, fe_%s_gfx950.inc)."
               % (mads, mads - n, n, dropped(body), body))
    out += emit_body(body, False, top31=True)
    return "\n".join(out) + "\n"


def outputs():
    """file name -> (text, summary line) of everything this tool writes"""
    out = {}
    for top31 in (False, True):
        for body in BODIES:
            name = "fe_%s_%sgfx950.inc" % (body, "t31_" if top31 else "")
            cols = schedule(body, top31=top31)
            mads = sum(len(c.terms) for c in cols)
            n = dropped(body, top31)
            out[name] = (render_t31(body) if top31 else render(body),
                         "%s: %d v_mad_u64_u32, %d v_addc_co_u32 (%d dropped; per column %s)"
                         % (name, mads, mads - n, n, " ".join(str(sum(1 for t in c.terms if not t.carry)) for c in cols)))
    return out


def render(body):
    mads = sum(len(c.terms) for c in schedule(body))
    out = list(HEADERS[body])
    out.append("// Nothing is assumed about the operands beyond 256 bits.  %d v_mad_u64_u32, %d v_addc_co_u32: %d carry adds dropped where the"
               % (mads, mads - dropped(body), dropped(body)))
    out.append("// bound of the 64-bit accumulator (exact integers, modulus limbs at their maximum over both fields) stays below 2^64.")
    out.append("#ifdef VDF_FE_CARRY_ALL     // A/B build only: every product followed by its carry add, the schedule before the bound argument")
    out += emit_body(body, True)
    out.append("#else")
    out += emit_body(body, False)
    out.append("#endif")
    return "\n".join(out) + "\n"


# ---- the emitted schedule as an integer model --------------------------------------------------------------------------------
def model_inputs(body, field, *operands):
    """operand names -> uint64 arrays of 32-bit words.  operands: numpy arrays of shape (n, 8), little-endian 32-bit limbs"""
    import numpy as np
    vals = {}
    for letter, arr in zip("abcd", operands):
        arr = np.asarray(arr, dtype=np.uint64)
        for i in range(8):
            vals["%s%d" % (letter, i)] = arr[:, i]
    if body == "sqr":                                  # fe_sqr_lazy's shifted limbs (fe.cuh)
        a = [vals["a%d" % i] for i in range(8)]
        for j in range(1, 8):
            vals["s%d" % j] = (a[j] << np.uint64(1)) & np.uint64(B32)
        for j in range(2, 8):
            vals["d%d" % j] = ((a[j] << np.uint64(1)) | (a[j - 1] >> np.uint64(31))) & np.uint64(B32)
        vals["d8"] = a[7] >> np.uint64(31)
    ml = limbs(MODULI[field])
    n = len(vals["a0"])
    for i in (1, 2, 3, 7):
        vals["m%d" % i] = np.full(n, ml[i], dtype=np.uint64)
    return vals


def model(cols, vals):
    """run a schedule on uint64 arrays: acc wraps at 64 bits, hi counts a carry only where a carry add is emitted, and a
    dropped carry add asserts that its multiply-add did not overflow.  Returns (r[0..7], ninth word, q[0..7])"""
    import numpy as np
    u = np.uint64
    n = len(vals["a0"])
    vals = dict(vals)
    acc = np.zeros(n, dtype=u)
    r = []
    for col in cols:
        hi = np.zeros(n, dtype=u)
        for t in col.terms:
            x, y = vals[t.x], vals[t.y]
            assert int(x.max()) <= B32 and int(y.max()) <= B32
            new = acc + x * y                          # both factors are 32-bit words: the product is exact, the sum wraps
            carry = new < acc
            if t.carry:
                hi = hi + carry.astype(u)
            else:
                assert not carry.any(), "column %d: %r overflowed the accumulator with its carry add dropped" % (col.k, t)
            acc = new
        lo, mid = acc & u(B32), acc >> u(32)
        if col.k < 8:
            vals["q%d" % col.k] = (u(1 << 32) - lo) & u(B32)
            nlo = mid + (lo != 0).astype(u)
            nmid = hi + (nlo >> u(32))
            assert int(nmid.max()) <= B32
            acc = (nmid << u(32)) | (nlo & u(B32))
        else:
            r.append(lo)
            assert int(hi.max()) <= B32
            acc = (hi << u(32)) | mid
    r.append(acc & u(B32))
    return r, acc >> u(32), [vals["q%d" % k] for k in range(8)]


def main(argv):
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vdf_amd", "csrc")
    check, bad = "--check" in argv, []
    for name, (text, summary) in outputs().items():
        path = os.path.join(root, name)
        if check:
            if not os.path.exists(path) or open(path).read() != text:
                bad.append(os.path.relpath(path))
        else:
            open(path, "w").write(text)
        print(summary)
    if bad:
        print("differs from what tools/gen_fe_mul.py generates: " + ", ".join(bad))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
