// Periodic rows (include/vdf_hip.h vdf_periodic_rows, vdf_nifs_cross_term_periodic): what makes a description and a call over it
// valid -- stated ONCE, header-only, as tape_rules.h states the rules of a tape: libvdf_hip.so's launcher (rounds.hip
// vec_nifs_cross_periodic) and libvdf_nova.so's host restatement (host/rounds_host.cpp eval_periodic_rows) include this file, since
// neither library can call the other's internals.  Host code only.  Both run a description this check has passed WITHOUT looking
// again: everything it could index out of range is refused here.  Where the pointers must live, and the vectors that may not be
// null, is each caller's own check.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/vdf_hip.h"

namespace vdfperiodic {

// "" to go on, else which rule failed (every one is VDF_ERR_BAD_ARG).  *nothing: reps = 0, the call is over and has done nothing.
inline std::string refuse(const vdf_periodic_rows* pr, uint64_t j_first, uint64_t reps, size_t seg_begin, size_t row0, size_t num_cols,
                          size_t num_cons, bool* nothing) {
  *nothing = false;
  if (!pr || !pr->row_start || (pr->n_terms && !pr->terms) || (pr->n_consts && !pr->consts)) return "null description";
  if (pr->n_cons == 0 || pr->n_cons > VDF_PERIODIC_MAX_ROWS || pr->n_vars == 0 || pr->n_terms > VDF_PERIODIC_MAX_TERMS ||
      pr->n_consts > VDF_PERIODIC_MAX_CONSTS)
    return "periodic rows exceed a published cap (VDF_PERIODIC_MAX_*), or have no row or variable";
  if (pr->row_start[0] != 0 || pr->row_start[3 * pr->n_cons] != pr->n_terms) return "row_start does not span the terms";
  for (uint32_t q = 0; q < 3 * pr->n_cons; ++q)
    if (pr->row_start[q + 1] < pr->row_start[q] || pr->row_start[q + 1] - pr->row_start[q] > VDF_PERIODIC_MAX_ROW_TERMS)
      return "row_start descends, or a row has more than VDF_PERIODIC_MAX_ROW_TERMS terms in one matrix";
  if (j_first < pr->j0) return "j_first lies before the repetition the pattern was taken from";
  if (reps == 0) { *nothing = true; return ""; }
  if (reps > ((uint64_t)1 << 31) / pr->n_cons || j_first > UINT32_MAX || j_first + reps > UINT32_MAX) return "more than 2^31 rows, or repetitions beyond 2^32";
  const uint64_t rows = reps * pr->n_cons, j_last = j_first + reps - 1;
  if (row0 > num_cons || rows > num_cons - row0) return "the row range ends beyond num_cons";
  if (num_cols == 0 || num_cols > ((size_t)1 << 32) || seg_begin > num_cols) return "num_cols out of range, or seg_begin beyond it";
  // (j < 2^32, n_vars < 2^32, seg_begin <= 2^32: the products stay inside 64 bits, and below 2^34 where a SEG term is admitted)
  const bool seg_far = j_last * pr->n_vars > ((uint64_t)1 << 33);      // (then no offset of 32 bits brings a SEG term back inside)
  const int64_t first_seg = (int64_t)(seg_begin + j_first * pr->n_vars), last_seg = (int64_t)(seg_begin + j_last * pr->n_vars);
  for (size_t e = 0; e < pr->n_terms; ++e) {
    const vdf_periodic_term& t = pr->terms[e];
    const std::string at = "term " + std::to_string(e);
    if (t.kind != VDF_TERM_SEG && t.kind != VDF_TERM_ABS) return at + ": unknown kind";
    if (t.c0 >= pr->n_consts || (t.c1 != VDF_TERM_NO_SLOPE && (t.c1 >= pr->n_consts || t.kind != VDF_TERM_ABS)))
      return at + ": constant index out of range, or a slope on a SEG term";
    if (t.kind == VDF_TERM_ABS) {
      if (t.col >= num_cols) return at + ": column beyond num_cols";
    } else {
      const int64_t rel = (int32_t)t.col;
      if (seg_far || first_seg + rel < 0 || last_seg + rel >= (int64_t)num_cols)
        return at + ": reaches a column outside [0, num_cols) in the first or the last repetition";
    }
  }
  return "";
}

}  // namespace vdfperiodic
