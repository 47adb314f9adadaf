// Round tapes (include/vdf_hip.h vdf_round_tape): what makes a tape valid in each of its three uses, and what one round of it
// costs -- stated ONCE, header-only, as pow_chain.h states a chain's rules: libvdf_hip.so's launchers (rounds.hip pack_tape) and
// libvdf_nova.so's host evaluators (host/rounds_host.cpp) include this file, since neither library can call the other's
// internals.  Host code only: no kernel reads this.  Both interpreters run a tape this check has passed WITHOUT looking again:
// everything a tape could index out of range is refused here -- opcodes, slots against n_slots, columns, constants, invariants
// and variables against their counts, reads of slots nothing has written, variables written twice or never.
#pragma once
#include "pow_chain.h"

namespace vdftape {

// ROUND: vdf_round_tape_run -- an ADV reads entry j (b = 0) or j + 1 (b = 1).  The walks write one advice entry per round
// (n_vars == n_adv) and may not load the entry being produced: WALK (vdf_round_tape_walk, descending) stands on entry j + 1,
// b = 1 only; FORWARD (vdf_round_tape_forward_walk) stands on entry j, b = 0 only.  POW and POWC are ops of FORWARD tapes only.
// TAB is an op of all three, in a tape that has a table: where the table lives (device-readable memory for a launcher, host memory
// for an evaluator) is the caller's to check -- here it is only not null.
enum Mode { ROUND, WALK, FORWARD };

struct Info {
  uint64_t products;       // the field products of one round, a POW or POWC counted as its squarings and multiplications; >= 1
  uint32_t chain_tmp;      // the largest n_tmp of the tape's chains (the slots a POWC keeps behind the two entries); 0: no POWC
  bool tab;                // the tape holds a TAB: it launches the kernels that admit one
};

// what square-and-multiply from the top set bit spends on exponent e: bitlen - 1 squarings and popcount - 1 products, at least one
inline uint64_t pow_products(const vdf_fe& e) {
  uint64_t bits = 0, ones = 0;
  for (int q = 0; q < 4; ++q)
    if (e.l[q]) { bits = 64 * q + 64 - __builtin_clzll(e.l[q]); ones += __builtin_popcountll(e.l[q]); }
  return bits + ones > 2 ? bits + ones - 2 : 1;
}

// "" for a tape that is valid in `mode` (*out filled, if asked for), else which rule failed, naming the op or the variable
inline std::string check(const vdf_round_tape* tp, Mode mode, Info* out) {
  if (!tp || (tp->n_ops && !tp->ops) || (tp->n_consts && !tp->consts)) return "null tape";
  if (tp->n_ops > VDF_TAPE_MAX_OPS || tp->n_consts > VDF_TAPE_MAX_CONSTS || tp->n_slots > VDF_TAPE_MAX_SLOTS || tp->n_vars > VDF_TAPE_MAX_VARS ||
      tp->n_inv > VDF_TAPE_MAX_INV || tp->n_adv > VDF_TAPE_MAX_ADV || tp->n_vars == 0 || tp->n_adv == 0 || tp->n_slots == 0)
    return "tape exceeds a published cap (VDF_TAPE_MAX_*), or has no variable, slot or advice column";
  if (mode != ROUND && tp->n_vars != tp->n_adv) return "walk tape: n_vars != n_adv (a round writes one advice entry)";
  if ((tp->tab_rows == 0) != (tp->tab_cols == 0)) return "tape table: tab_rows and tab_cols are both 0 (no table) or both positive";
  if (tp->tab_rows > VDF_TAPE_MAX_TAB_ROWS || tp->tab_cols > VDF_TAPE_MAX_TAB_COLS)
    return "tape table exceeds a published cap (VDF_TAPE_MAX_TAB_ROWS, VDF_TAPE_MAX_TAB_COLS)";
  if (tp->tab_rows && !tp->table) return "tape table: null table with tab_rows > 0";
  bool written[VDF_TAPE_MAX_SLOTS] = {}, var_out[VDF_TAPE_MAX_VARS] = {};
  Info info = {0, 0, false};
  for (size_t i = 0; i < tp->n_ops; ++i) {
    const vdf_tape_op& o = tp->ops[i];
    auto rd = [&](uint8_t x) { return x < tp->n_slots && written[x]; };
    bool ok = false;
    switch (o.op) {
      case VDF_TAPE_ADV: ok = o.a < tp->n_adv && (mode == WALK ? o.b == 1 : mode == FORWARD ? o.b == 0 : o.b <= 1); break;
      case VDF_TAPE_INV: ok = o.a < tp->n_inv; break;
      case VDF_TAPE_J: ok = true; break;
      case VDF_TAPE_CONST: ok = o.a < tp->n_consts; break;
      case VDF_TAPE_ADD: case VDF_TAPE_SUB: ok = rd(o.a) && rd(o.b); break;
      case VDF_TAPE_MUL: ok = rd(o.a) && rd(o.b); ++info.products; break;
      case VDF_TAPE_SCALE: ok = rd(o.a) && o.b < tp->n_consts; ++info.products; break;
      case VDF_TAPE_OUT: ok = rd(o.a) && o.b < tp->n_vars && !var_out[o.b]; if (ok) var_out[o.b] = true; break;
      case VDF_TAPE_POW:
        ok = mode == FORWARD && rd(o.a) && o.b < tp->n_consts;
        if (ok) info.products += pow_products(tp->consts[o.b]);
        break;
      case VDF_TAPE_POWC:
        ok = mode == FORWARD && rd(o.a);
        if (ok) {
          vdfpow::ChainInfo ci;
          const std::string why = vdfpow::check_packed(tp->consts, tp->n_consts, o.b, &ci, nullptr, nullptr);
          if (!why.empty()) return "tape op " + std::to_string(i) + ": the chain of a POWC: " + why;
          info.products += ci.products();
          if (ci.n_tmp > info.chain_tmp) info.chain_tmp = ci.n_tmp;
        }
        break;
      case VDF_TAPE_TAB:
        if (tp->tab_rows == 0) return "tape op " + std::to_string(i) + " is malformed: a TAB in a tape without a table (tab_rows = 0)";
        if (o.a >= tp->tab_cols) return "tape op " + std::to_string(i) + ": a TAB of column " + std::to_string(o.a) + " >= tab_cols";
        if (o.b != 0) return "tape op " + std::to_string(i) + ": a TAB with b != 0";
        ok = info.tab = true;
        break;
      default: break;
    }
    if (ok && o.op != VDF_TAPE_OUT) { ok = o.dst < tp->n_slots; if (ok) written[o.dst] = true; }
    if (!ok)
      return "tape op " + std::to_string(i) + " is malformed (opcode, index out of range, or a slot read before it is written)" +
             (mode == WALK ? "; a walk tape loads advice with b = 1 only" : mode == FORWARD ? "; a forward walk tape loads advice with b = 0 only" : "");
  }
  for (uint32_t v = 0; v < tp->n_vars; ++v)
    if (!var_out[v]) return "tape leaves variable " + std::to_string(v) + " unwritten";
  if (info.products == 0) info.products = 1;
  if (out) *out = info;
  return "";
}

}  // namespace vdftape
