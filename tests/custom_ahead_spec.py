"""Circuits and a model for a custom chain's lookahead and early rows (include/vdf_nova.h tuning.custom_ahead, THE PROBE).

FC     custom_chain_spec's circuit: inv = [i_in], carry_in = [x, y], all of them z_in -- the early rows are the repeat's 3t rows.
FCgap  FC with one variable of its own allocated between z_in and the repeat: the same rows, the segment one column further on.
FCown  FC whose inv is a variable of its own (cs.alloc), constrained equal to i_in: its rows read a variable that is neither z_in
       nor the segment, so it has no early rows.  lie = True: the value is i_in + 1 in a probe synthesis (cs.is_probe), so every
       lookahead is made with an inv the real step does not have -- a miss, every step.

early_run_model: the rule of vdf_nova_shape_early_rows_custom over the triples of shape_export_custom, in numpy."""
import numpy as np

from custom_chain_spec import FC
from rounds_spec import MOD
from oracle import pasta as o


class FCgap(FC):
    def synthesize(self, cs, z):
        cs.alloc(self.fe(5) if cs.is_witness else None)
        return super().synthesize(cs, z)


class FCown(FC):
    lie = False

    def synthesize(self, cs, z):
        x, y, i_in = z
        val = None
        if cs.is_witness:
            v = o.from_mont(int.from_bytes(cs.value(i_in), "little"), self.m)
            val = self.fe(v + (1 if self.lie and cs.is_probe else 0))
        own = cs.alloc(val)
        cs.enforce(own, cs.const(self.fe(1)), i_in)
        adv = None
        if cs.is_witness:
            adv = self.advice if self.advice is not None else cs.step_advice()
        self.seen.append((cs.is_witness, cs.step_advice()))
        x, y = cs.repeat(self.body(), self.t, [own], [x, y], adv)
        return [x, y, cs.add(i_in, cs.const(self.fe(self.t)))]


class FCliar(FCown):
    lie = True


def early_run_model(mats, num_cons, num_vars, seg_begin, seg_len, zin_begin, arity, floor=64, row_cap=8):
    """(first row, rows) of the longest run of rows that read only [seg_begin, seg_begin + seg_len), [zin_begin, zin_begin + arity)
    and the constant column num_vars, no row with more than row_cap entries in a matrix; (0, 0) below `floor` rows"""
    early = np.ones(num_cons, dtype=bool)
    for rows, cols, _ in mats:
        rows, cols = rows.astype(np.int64), cols.astype(np.int64)
        ok = ((cols >= seg_begin) & (cols < seg_begin + seg_len)) | ((cols >= zin_begin) & (cols < zin_begin + arity)) | (cols == num_vars)
        early[rows[~ok]] = False
        early[np.bincount(rows, minlength=num_cons) > row_cap] = False
    best_b = best_n = run_b = 0
    for r in range(num_cons + 1):
        if r == num_cons or not early[r]:
            if r - run_b > best_n:
                best_b, best_n = run_b, r - run_b
            run_b = r + 1
    return (best_b, best_n) if best_n >= floor else (0, 0)


def cols_of_row(mat, row):
    rows, cols, _ = mat
    return sorted(int(c) for c in cols[rows == row])
