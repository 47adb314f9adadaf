"""The big-integer statement of the multi-point sparse evaluation (include/vdf_hip.h vdf_sparse_eval_multi; the batch verifier's
M(r_x, r_y) of many compressed proofs in one pass over a shape's rows).  Host only: plain Python integers, no GPU import.

    out[q] = sum over the entries (x, y, v) of A, B, C of  eq_x[q][x] * w_q(matrix) * v * eq_y[q][ycol(y)]  mod m,
    w_q = 1, rho[q], rho[q]^2,    ycol(y) = y for y < col_split, else col_hi_base + (y - col_split).

A matrix is a list of (row, column, value) triples of plain integers (oracle.pasta.R1CSShape's A, B, C); repeated (row, column)
entries add up.  The vectors are arbitrary: nothing here knows that the verifier passes eq tables.  tests/test_sparse_eval_spec.py
pins the column map and the index order to what oracle/spartan.py's verifier uses.  The code under test is never an input."""


def ycol(y, col_split, col_hi_base):
    return y if y < col_split else col_hi_base + (y - col_split)


def multi_eval(mats, m, eq_xs, eq_ys, rhos, col_split, col_hi_base):
    """[out[q]] for the instances (eq_xs[q], eq_ys[q], rhos[q]); mats = (A, B, C)."""
    assert len(mats) == 3 and len(eq_xs) == len(eq_ys) == len(rhos)
    mapped = [[(r, ycol(c, col_split, col_hi_base), v) for r, c, v in mat] for mat in mats]
    out = []
    for ex, ey, rho in zip(eq_xs, eq_ys, rhos):
        s = [sum(ex[r] * v * ey[c] for r, c, v in mat) for mat in mapped]
        out.append((s[0] + rho * s[1] + rho * rho * s[2]) % m)
    return out


def pow2_at_least(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def layout_of(num_vars, num_io):
    """The padded column layout of the compression argument: z = [W | u | X] with W at [0, NW) and (u, X) from NW on, Z = 2 NW
    columns in all.  Returns NW, Z and the column map as vdf_sparse_eval_multi takes it."""
    NW = pow2_at_least(num_vars)
    assert 1 + num_io <= NW
    return {"NW": NW, "Z": 2 * NW, "col_split": num_vars, "col_hi_base": NW, "num_cols": num_vars + 1 + num_io}
