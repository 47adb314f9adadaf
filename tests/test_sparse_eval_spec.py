"""CPU: tests/sparse_eval_spec.py against oracle/spartan.py.  With eq tables as inputs and the verifier's split of the columns, the
spec's value is the M(r_y) that spartan.verify computes as  sum_y m_vector(shape, eq(r_x, .), rho, NW, q)[y] * eq(r_y, .)[y]  -- which
pins the column map (W at [0, NW), u and X from NW) and the MSB-first index order of the tables to what the verifier uses."""
import random

import pytest

from oracle import nova as nv, pasta as o, spartan as sp
import sparse_eval_spec as E


def _cubic_shape():
    """the cubic circuit of the seam's tests (z -> z^3 + z + 5) with its input and output exposed"""
    cs = nv.CS(o.FIELD_FQ)
    x = cs.alloc(7)
    cs.enforce_equal(x, cs.alloc_io(7))
    (y,) = nv.CubicCircuit().synthesize(cs, [x])
    cs.enforce_equal(y, cs.alloc_io(y.v))
    return cs.shape()


SHAPES = {"minroot_t3_fq": (lambda: o.step_circuit_shape(3, o.FIELD_FQ), o.Q),
          "minroot_t3_fp": (lambda: o.step_circuit_shape(3, o.FIELD_FP), o.P),
          "cubic": (_cubic_shape, o.Q)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_spec_is_the_verifiers_m_of_ry(name):
    make, q = SHAPES[name]
    shape = make()
    M, NW, Z = sp._layout(shape)
    lay = E.layout_of(shape.num_vars, shape.num_io)
    assert (lay["NW"], lay["Z"]) == (NW, Z)
    assert all(E.ycol(c, lay["col_split"], lay["col_hi_base"]) == sp._col(shape, NW, c) for c in range(lay["num_cols"]))
    s, l1 = M.bit_length() - 1, Z.bit_length() - 1
    rng = random.Random(name)
    eq_xs, eq_ys, rhos, want = [], [], [], []
    for case in range(4):
        rx = [rng.randrange(q) for _ in range(s)]
        ry = [rng.randrange(q) for _ in range(l1)]
        rho = (0, 1, q - 1, rng.randrange(q))[case]
        eq_rx, eq_ry = sp.eq_table(rx, q), sp.eq_table(ry, q)
        mv = sp.m_vector(shape, eq_rx, rho, NW, q)
        want.append(sum(a * b for a, b in zip(mv, eq_ry)) % q)
        eq_xs.append(eq_rx); eq_ys.append(eq_ry); rhos.append(rho)
    got = E.multi_eval((shape.A, shape.B, shape.C), q, eq_xs, eq_ys, rhos, lay["col_split"], lay["col_hi_base"])
    assert got == want
    assert len(set(got)) == 4 and all(got)


def test_index_order_is_msb_first():
    """a boolean point picks one entry of each table: r_x = the bits of a row, r_y = the bits of a padded column, first bit the
    most significant -- the spec's value is then that row's entry sum at that column"""
    shape = o.step_circuit_shape(3, o.FIELD_FQ)
    q = o.Q
    M, NW, Z = sp._layout(shape)
    lay = E.layout_of(shape.num_vars, shape.num_io)
    s, l1 = M.bit_length() - 1, Z.bit_length() - 1
    bits = lambda v, k: [(v >> (k - 1 - j)) & 1 for j in range(k)]
    rho = 3
    for r, c, v in (shape.A[0], shape.A[-1], shape.B[1]):
        y = sp._col(shape, NW, c)
        got = E.multi_eval((shape.A, shape.B, shape.C), q, [sp.eq_table(bits(r, s), q)], [sp.eq_table(bits(y, l1), q)], [rho],
                           lay["col_split"], lay["col_hi_base"])[0]
        want = sum(w * vv for w, mat in ((1, shape.A), (rho, shape.B), (rho * rho, shape.C)) for rr, cc, vv in mat if (rr, cc) == (r, c)) % q
        assert got == want and want != 0


def test_identity_map_and_arbitrary_vectors():
    mats = ([(0, 0, 2), (0, 2, 3), (1, 2, 5), (1, 2, 7)], [(1, 1, 11)], [(0, 2, 13)])
    m = 10007
    ex, ey = [[3, 4]], [[5, 6, 7]]
    assert E.multi_eval(mats, m, ex, ey, [2], 3, 0) == [(3 * (2 * 5 + 3 * 7) + 4 * (12 * 7) + 2 * 4 * 11 * 6 + 4 * 3 * 13 * 7) % m]
    # columns 2.. moved to 4..: the split leaves a gap the entries never read
    ey2 = [[5, 6, 999, 999, 7]]
    assert E.multi_eval(mats, m, ex, ey2, [2], 2, 4) == E.multi_eval(mats, m, ex, ey, [2], 3, 0)
