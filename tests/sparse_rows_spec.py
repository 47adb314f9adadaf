"""Shared by the tests of the kernels that walk the CSR rows of a vdf_shape (vdf_amd/csrc/vecops.hip: k_spmv, k_spmv_long,
k_nifs_cross, k_nifs_cross_w<4>, k_nifs_cross_w<8>, k_nifs_cross_f, k_relaxed_residual_batch): a deterministic shape whose row
lengths are CHOSEN per matrix, the census that names every feature the shape was built to have, the row ranges the range calls
are tried on, the rule that says which kernels a call launches, and the big-integer references.  Host only: no GPU import.

The shape.  Per-matrix row lengths come from LENGTHS.  A row is long when one of its matrices has more than LONG_ROW = 8 entries
(VDF_LONG_ROW, vdf_amd/csrc/internal.h): a wavefront sums it.  Long rows sit at 0, 31, 32, 63, 64, 255, 256 and num_cons - 1, at
whatever `extra_long` adds, and at as many of FILL_LONG as make every combination of LONG_COMBOS appear and the number of long
rows 1 mod 4 (the last workgroup of four wavefronts is then partly empty).  Every other row is short: the combinations of
SHORT_COMBOS three times over from the first short row on, then lengths drawn from 0 .. 8.  Coefficients are +1, -1 (the two
the kernels add and subtract without a product) and general values, 2 and m - 2 among them; every long row holds all three kinds.
Columns include 0 and the last one; a few rows repeat a column within one matrix -- vdf_shape_create keeps duplicates as separate
entries, so both the kernels and the reference add them up.

The references are plain Python integers with oracle.pasta's Montgomery conversions.  The code under test is never an input."""
import numpy as np

from oracle import pasta as o
from util import ints, limbs

LONG_ROW = 8                                   # VDF_LONG_ROW
LANE_LIMIT = 1 << 15                           # nifs_cross_lanes(rows): 8 lanes per row up to here, 1 above
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 300)
SHORT_LENGTHS = tuple(x for x in LENGTHS if x <= LONG_ROW)
FIXED_LONG = (0, 31, 32, 63, 64, 255, 256)     # and num_cons - 1
FILL_LONG = (257, 384, 385, 511, 640)
ROWS_ALL, ROWS_INSIDE, ROWS_OUTSIDE = 0, 1, 2  # VDF_ROWS_* (include/vdf_hip.h)

# (A, B, C) lengths of the long rows, dealt to the long positions in ascending order, round and round
LONG_COMBOS = ((300, 300, 300), (129, 9, 0), (0, 257, 64), (9, 0, 0), (0, 9, 0), (0, 0, 9), (8, 8, 9), (10, 63, 65),
               (127, 128, 191), (192, 193, 256), (64, 1, 129), (256, 3, 5), (65, 0, 300))
# k_nifs_cross and k_relaxed_residual_batch prefetch PRE = {2, 2, 4} entries of A, B, C: the tail loop starts at 3, 3 and 5
SHORT_COMBOS = ((3, 1, 1), (8, 1, 1), (1, 3, 1), (1, 8, 1), (1, 1, 5), (1, 1, 8), (8, 8, 8), (0, 0, 0), (2, 2, 4), (3, 3, 5),
                (1, 0, 0), (0, 1, 0), (0, 0, 1), (4, 5, 7), (7, 4, 2), (8, 0, 3), (0, 8, 8), (5, 7, 0), (1, 1, 1), (2, 2, 5))
PRE = (2, 2, 4)
N_GENERAL = 64                                 # distinct general coefficients (a circuit's dictionary is small too)


def long_positions(num_cons, extra_long=()):
    pos = sorted(set(FIXED_LONG) | {num_cons - 1} | set(int(x) for x in extra_long))
    assert pos[-1] == num_cons - 1 and num_cons > FIXED_LONG[-1] + 2
    for f in FILL_LONG:
        if len(pos) >= len(LONG_COMBOS) and len(pos) % 4 == 1:
            break
        if f < num_cons - 1 and f not in pos:
            pos = sorted(pos + [f])
    assert len(pos) >= len(LONG_COMBOS) and len(pos) % 4 == 1, (num_cons, pos)
    return pos


def _distinct_short_cols(rng, lens, num_cols):
    """int64[n, 8]: the first lens[r] entries of row r are distinct columns"""
    n = len(lens)
    c = rng.integers(0, num_cols, size=(n, LONG_ROW))
    j = np.arange(LONG_ROW)
    s = np.sort(np.where(j[None, :] < lens[:, None], c, num_cols + j[None, :]), axis=1)
    for r in np.nonzero((s[:, 1:] == s[:, :-1]).any(axis=1))[0]:
        c[r, :lens[r]] = rng.choice(num_cols, size=int(lens[r]), replace=False)
    return c


def adversarial_shape(field, num_cons, seed, num_cols=701, extra_long=()):
    """([(rows uint32[nnz], cols uint32[nnz], vals uint64[nnz, 4] Montgomery)] x 3 as Context.shape_create takes them, census)."""
    m = o.modulus(field)
    rng = np.random.default_rng([seed, field, num_cons])
    longs = long_positions(num_cons, extra_long)
    lens = np.zeros((num_cons, 3), dtype=np.int64)
    is_long = np.zeros(num_cons, dtype=bool)
    is_long[longs] = True
    for i, r in enumerate(longs):
        lens[r] = LONG_COMBOS[i % len(LONG_COMBOS)]
    short = np.nonzero(~is_long)[0]
    fixed = min(len(short), 3 * len(SHORT_COMBOS))
    for i in range(fixed):
        lens[short[i]] = SHORT_COMBOS[i % len(SHORT_COMBOS)]
    lens[short[fixed:]] = rng.choice(SHORT_LENGTHS, size=(len(short) - fixed, 3))
    # coefficient values: index 0 is +1, 1 is -1, the rest general with 2 and m - 2 in front
    general = [2, m - 2] + [int(v) % m for v in ints(rng.integers(0, 2**64, size=(N_GENERAL - 2, 4), dtype=np.uint64))]
    assert all(1 < g < m - 1 for g in general)
    values = [1, m - 1] + general
    value_limbs = limbs([o.to_mont(v, m) for v in values])
    last = num_cols - 1
    mats, dup_rows = [], []
    for k in range(3):
        ln = lens[:, k]
        rowptr = np.concatenate([[0], np.cumsum(ln)])
        nnz = int(rowptr[-1])
        rows = np.repeat(np.arange(num_cons), ln).astype(np.uint32)
        cols = np.zeros(nnz, dtype=np.int64)
        sc = _distinct_short_cols(rng, np.minimum(ln, LONG_ROW), num_cols)
        within = np.arange(nnz) - np.repeat(rowptr[:-1], ln)                 # position of an entry inside its row
        short_entry = np.repeat(ln <= LONG_ROW, ln)
        cols[short_entry] = sc[rows[short_entry], within[short_entry]]
        kind = rng.integers(0, 4, size=nnz)                                   # +1, -1, general, general
        ci = np.where(kind < 2, kind, 2 + rng.integers(0, N_GENERAL, size=nnz))
        for i, r in enumerate(longs):
            n, lo = int(ln[r]), int(rowptr[r])
            if n > LONG_ROW:
                c = rng.permutation(num_cols)[:n]
                if i % 2 == 0:                                                # column 0 and the last column, each once
                    c = c[(c != 0) & (c != last)]
                    c = np.concatenate([[0, last], c])[:n]
                    c = c[rng.permutation(n)]
                if n >= 72 and i % 3 == 0:                                    # one column twice: two lanes, two passes of 64
                    c[70] = c[5]
                    dup_rows.append((k, int(r)))
                cols[lo:lo + n] = c
            if n >= 3:                                                        # all three kinds in every matrix of a long row
                at = rng.permutation(n)[:5]
                ci[lo + at] = [0, 1, 2, 3, 2 + int(rng.integers(2, N_GENERAL))][:len(at)]
        # short rows with a repeated column (prefetched entry and tail entry; two lanes of a group), with column 0, with the last
        for i, r in enumerate(short[:fixed]):
            n, lo = int(ln[r]), int(rowptr[r])
            if n == LONG_ROW and i < len(SHORT_COMBOS):
                cols[lo + n - 1] = cols[lo]
                dup_rows.append((k, int(r)))
            elif n >= 1 and len(SHORT_COMBOS) <= i < 2 * len(SHORT_COMBOS) and i % 2 == 0 and 0 not in cols[lo + 1:lo + n]:
                cols[lo] = 0
            elif n >= 2 and len(SHORT_COMBOS) <= i < 2 * len(SHORT_COMBOS) and last not in cols[lo:lo + n - 1]:
                cols[lo + n - 1] = last
        mats.append((rows, cols.astype(np.uint32), np.ascontiguousarray(value_limbs[ci])))
    return mats, census(mats, m, num_cons, num_cols, dup_rows)


def row_lengths(mats, num_cons):
    """int64[num_cons, 3]"""
    return np.stack([np.bincount(r, minlength=num_cons) for r, _, _ in mats], axis=1).astype(np.int64)


def unmont_unique(vals, m):
    """ints of uint64[n, 4] Montgomery values, converting each distinct value once"""
    raw, table, out = np.ascontiguousarray(vals, dtype="<u8").tobytes(), {}, []
    for i in range(0, len(raw), 32):
        b = raw[i:i + 32]
        v = table.get(b)
        if v is None:
            v = table[b] = o.from_mont(int.from_bytes(b, "little"), m)
        out.append(v)
    return out


def census(mats, m, num_cons, num_cols, dup_rows=()):
    """What the shape really holds, by name: the host test asserts every entry, so that an edit of the builder cannot hollow the
    GPU tests out.  Computed from the triples alone."""
    lens = row_lengths(mats, num_cons)
    combos = set(map(tuple, lens.tolist()))
    long_rows = np.nonzero((lens > LONG_ROW).any(axis=1))[0].tolist()
    is_long = set(long_rows)
    col_refs0, all_vals, all_cols = set(), set(), set()
    per_row_kinds = {r: set() for r in long_rows}
    dups = 0
    for k, (rows, cols, vals) in enumerate(mats):
        v = unmont_unique(vals, m)
        all_vals |= set(v)
        all_cols |= set(cols.tolist())
        for r, c, x in zip(rows.tolist(), cols.tolist(), v):
            if c == 0:
                col_refs0.add(r)
            if r in is_long:
                per_row_kinds[r].add("+1" if x == 1 else "-1" if x == m - 1 else "general")
        order = np.lexsort((cols, rows))
        dups += int(((rows[order][1:] == rows[order][:-1]) & (cols[order][1:] == cols[order][:-1])).sum())
    kinds_ok = all(s == {"+1", "-1", "general"} for s in per_row_kinds.values())
    passes = lambda n: (n + 127) // 128                                       # k_nifs_cross_f: passes of 128 entries
    runs, start = [], None
    for r in range(num_cons + 1):
        s = r < num_cons and r not in is_long
        if s and start is None:
            start = r
        if not s and start is not None:
            runs.append((start, r - start))
            start = None
    absent_slot_rows = [r for r in range(num_cons) if r not in is_long and r not in col_refs0 and
                        any(lens[r, k] < PRE[k] for k in range(3))]
    return {
        "num_cons": num_cons, "num_cols": num_cols, "long_rows": long_rows, "short_runs": runs,
        "lengths_used": sorted(set(lens.reshape(-1).tolist())),
        "lengths_all_from_the_set": set(lens.reshape(-1).tolist()) <= set(LENGTHS),
        "every_length_of_the_set": set(lens.reshape(-1).tolist()) == set(LENGTHS),
        "A_at_3_and_8_while_C_is_1": (3, 1, 1) in combos and (8, 1, 1) in combos,
        "B_at_3_and_8_while_C_is_1": (1, 3, 1) in combos and (1, 8, 1) in combos,
        "C_at_5_and_8_while_A_B_are_1": (1, 1, 5) in combos and (1, 1, 8) in combos,
        "all_three_at_8": (8, 8, 8) in combos,
        "nine_in_one_matrix_alone": all(c in combos for c in ((9, 0, 0), (0, 9, 0), (0, 0, 9))),
        "combo_129_9_0": (129, 9, 0) in combos, "combo_0_257_64": (0, 257, 64) in combos,
        "combo_300_300_300": (300, 300, 300) in combos, "combo_8_8_9": (8, 8, 9) in combos,
        "all_empty_row": (0, 0, 0) in combos,
        "long_and_empty_or_short_in_one_row": any(max(c) > LONG_ROW and min(c) == 0 for c in combos) and
                                              any(max(c) > LONG_ROW and 0 < min(c) <= LONG_ROW for c in combos),
        "passes_differ_within_a_long_row": any(len({passes(x) for x in c if x > 0}) > 1 for c in combos if max(c) > LONG_ROW),
        "three_passes": any(passes(max(c)) == 3 for c in combos),
        "long_at_fixed_positions": all(r in is_long for r in FIXED_LONG + (num_cons - 1,)),
        "adjacent_long_rows": any(r + 1 in is_long for r in long_rows),
        "long_rows_1_mod_4": len(long_rows) % 4 == 1,
        "long_row_matrix_pairs_not_0_mod_4": int((lens > LONG_ROW).sum()) % 4 != 0,      # k_spmv_long's list
        "short_rows_mixed_0_to_8": {x for r in range(num_cons) if r not in is_long for x in lens[r].tolist()} == set(SHORT_LENGTHS),
        "coefficient_kinds": {1, m - 1, 2, m - 2} <= all_vals and len(all_vals) > 8,
        "every_long_row_holds_all_kinds": kinds_ok,
        "column_0_and_last": 0 in all_cols and num_cols - 1 in all_cols,
        "repeated_columns": dups, "rows_built_with_a_repeat": list(dup_rows),
        "short_rows_with_an_absent_slot_and_no_column_0": len(absent_slot_rows),
        "longest_short_run": max(n for _, n in runs),
    }


REQUIRED = ("lengths_all_from_the_set", "every_length_of_the_set", "A_at_3_and_8_while_C_is_1", "B_at_3_and_8_while_C_is_1",
            "C_at_5_and_8_while_A_B_are_1", "all_three_at_8", "nine_in_one_matrix_alone", "combo_129_9_0", "combo_0_257_64",
            "combo_300_300_300", "combo_8_8_9", "all_empty_row", "long_and_empty_or_short_in_one_row",
            "passes_differ_within_a_long_row", "three_passes", "long_at_fixed_positions", "adjacent_long_rows", "long_rows_1_mod_4",
            "long_row_matrix_pairs_not_0_mod_4", "short_rows_mixed_0_to_8", "coefficient_kinds", "every_long_row_holds_all_kinds",
            "column_0_and_last", "repeated_columns", "short_rows_with_an_absent_slot_and_no_column_0")

# ---- the shapes of the GPU tests ------------------------------------------------------------------------------------------
# small: 769 = 1 mod 32, 64 and 256.  large: 33025 = 129 * 256 + 1, just above 2^15, long rows at 32767 and 32768 too.
# boundary: a run of MORE than 2^15 short rows does not fit into 33025 rows between the long rows at 256 and at 32767 (32510
# rows), nor with the two left out (257 .. 33023 are 32767 rows), so the INSIDE side of the 2^15 boundary has a shape of its
# own: 33537 = 131 * 256 + 1 rows under the same placement rule, with the short run 641 .. 33535 (32895 rows).
SHAPES = {"small": dict(num_cons=769, num_cols=701, extra_long=()),
          "large": dict(num_cons=33025, num_cols=2053, extra_long=(32767, 32768)),
          "boundary": dict(num_cons=33537, num_cols=2053, extra_long=())}
SEED = 20


def make_shape(name, field):
    return adversarial_shape(field, seed=SEED, **SHAPES[name])


def row_ranges(cen):
    """[(row_begin, row_count)] without a long row inside: every maximal run of short rows; the empty range at 0, in the middle and
    at num_cons; one row right after and right before a long row; starts and ends at a multiple of 32, of 64 and of 256 and at
    each of those +- 1 (511 and 513 are ends, 512 and 513 starts: 511 is a long row)."""
    n = cen["num_cons"]
    out = list(cen["short_runs"]) + [(0, 0), (n // 2, 0), (n, 0), (1, 1), (30, 1), (33, 1),
                                     (96, 32), (95, 34), (97, 30), (128, 64), (127, 66), (129, 62), (500, 11), (512, 1), (513, 127), (513, 0)]
    if n > 4096:
        out += [(1024, 1024), (1023, 1026), (1025, 1022), (32769, 1), (32700, 67)]
    longs = cen["long_rows"]
    for b, c in out:
        assert b + c <= n and not any(b <= r < b + c for r in longs), (b, c)
    return out


def expected_labels(part, row_count, cen, nifs_lanes, nifs_fused):
    """The timed launches of vdf_nifs_cross_term (part ALL) / vdf_nifs_cross_term_rows, as include/vdf_hip.h and the tuning's
    description state them: eight lanes per row up to 2^15 rows of the launch and one above unless nifs_lanes forces 1, 4 or 8;
    the long rows inside the launch (k_nifs_cross_f) when it runs eight lanes and nifs_fused is set, else by k_spmv_long ahead
    of it; an INSIDE range holds no long row; a launch over no rows does not happen."""
    n = cen["num_cons"]
    rows = n if part == ROWS_ALL else (row_count if part == ROWS_INSIDE else n - row_count)
    lanes = nifs_lanes if nifs_lanes in (1, 4, 8) else (8 if rows <= LANE_LIMIT else 1)
    has_long = part != ROWS_INSIDE and len(cen["long_rows"]) > 0
    if rows == 0:
        return ["k_spmv_long"] if has_long and not (nifs_fused and lanes == 8) else []
    if has_long and nifs_fused and lanes == 8:
        return ["k_nifs_cross_f"]
    cross = {1: "k_nifs_cross", 4: "k_nifs_cross_w4", 8: "k_nifs_cross_w8"}[lanes]
    return (["k_spmv_long"] if has_long else []) + [cross]


# ---- big-integer references -------------------------------------------------------------------------------------------------
def products(mats, m, num_cons, z):
    """[A z, B z, C z] as lists of ints below m; z a list of ints.  Repeated (row, column) entries add up."""
    out = []
    for rows, cols, vals in mats:
        acc = [0] * num_cons
        for r, c, v in zip(rows.tolist(), cols.tolist(), unmont_unique(vals, m)):
            acc[r] += v * z[c]
        out.append([x % m for x in acc])
    return out


def cross_term(a1, b1, c1, a2, b2, c2, u1, m):
    """T = a1 b2 + a2 b1 - u1 c2 - c1 (the second instance is fresh: u2 = 1)"""
    return [(x1 * y2 + x2 * y1 - u1 * w2 - w1) % m for x1, y1, w1, x2, y2, w2 in zip(a1, b1, c1, a2, b2, c2)]


def residual(mats, m, zs, Es, us, rhos, num_cons=None, prods=None):
    """out[r] = sum_q rho_q ((A z_q)[r] (B z_q)[r] - u_q (C z_q)[r] - E_q[r]) (the comment above k_relaxed_residual_batch); Es is
    None or a list whose entries may be None (the zero vector); rho_q a plain integer.  num_cons: by default the largest row of
    the triples plus one.  prods: products(mats, m, num_cons, z) of each z, where a caller has them already."""
    if num_cons is None:
        num_cons = 1 + max(int(r.max()) for r, _, _ in mats if len(r))
    out = [0] * num_cons
    for q, z in enumerate(zs):
        a, b, c = prods[q] if prods is not None else products(mats, m, num_cons, z)
        E = Es[q] if Es is not None else None
        u, rho = us[q], rhos[q]
        for r in range(num_cons):
            out[r] += rho * (a[r] * b[r] - u * c[r] - (E[r] if E is not None else 0))
    return [x % m for x in out]


def rand_ints(rng, m, n):
    """n uniformly random 254-bit integers (all below both moduli)"""
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    v = ints(a)
    assert all(x < m for x in v)
    return v


def lengths_table(mats, num_cons):
    """{matrix letter: sorted row lengths that occur} of a shape's triples"""
    lens = row_lengths(mats, num_cons)
    return {"ABC"[k]: sorted(set(lens[:, k].tolist())) for k in range(3)}
