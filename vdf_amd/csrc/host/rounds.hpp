// Uniform rounds of a custom step circuit (include/vdf_nova.h vdf_cs_repeat): the body as recorded, its replay over a constraint
// system, and the slot-allocated program the GPU runs (include/vdf_hip.h vdf_round_tape).  rounds_host.cpp.
#pragma once
#include <cstring>
#include <vector>
#include "../../../include/vdf_nova.h"
#include "r1cs.hpp"

namespace vdfnova {

// What a body did, call by call.  Nodes [0, n_inputs()) are its inputs in the order j, inv, carry, cur, next; every later node is
// one vdf_cs_* call.  a, b, c name nodes, except: R_CONST a = index into consts; R_SCALE and R_POW b = index into consts (R_POW:
// the exponent, a plain 256-bit integer, stored like a constant).  R_POWC (vdf_cs_pow_chain): b = index of the first of the
// constants the packed chain lies in (csrc/pow_chain.h), c = its n_tmp.  R_POW and R_POWC exist in forward bodies only.
// R_TAB (vdf_cs_tab): a = the column of the record's one table; the round constant table[j mod rows][a] -- in a round body a
// constant like j (replay_round puts its value on the constant's column), in walk and forward bodies a value.
enum RecOp : uint8_t { R_INPUT = 0, R_CONST, R_ADD, R_SUB, R_SCALE, R_MUL, R_ALLOC_FROM, R_ENFORCE, R_POW, R_POWC, R_TAB };
struct RecNode {
  uint8_t op = R_INPUT;
  bool value_only = false;         // made of advice values: no linear combination stands behind it
  uint32_t a = 0, b = 0, c = 0;
  bool operator==(const RecNode& o) const { return op == o.op && value_only == o.value_only && a == o.a && b == o.b && c == o.c; }
};
struct RoundRecord {
  uint32_t n_inv = 0, n_carry = 0, n_adv = 0;
  std::vector<RecNode> nodes;
  std::vector<Fe> consts;
  std::vector<uint32_t> carry_out;                 // nodes
  uint32_t n_vars = 0, n_cons = 0;                 // per repetition
  // the device program (compile()): inputs loaded at their first use, slots by a linear scan over live ranges
  std::vector<vdf_tape_op> ops;
  uint32_t n_slots = 0;
  uint32_t chain_tmp = 0;                          // the largest n_tmp of the POWCs the program holds (slots behind the two entries)
  // the body's one table (vdf_cs_tab): the caller's pointer, which identifies it while the body records and which the caller
  // keeps alive for as long as the record is used -- a recording copies nothing (a body is recorded again in every step).  A
  // record that OUTLIVES the call it was made in (the parameters') takes its own copy once: keep_table().  same_body compares the
  // elements, wherever they lie: one pass over at most 1 MiB per step, the price of "another table is another circuit".
  const vdf_fe* tab_src = nullptr;
  uint32_t tab_rows = 0, tab_cols = 0;
  std::vector<Fe> table;                           // keep_table()'s copy, else empty
  size_t tab_elems() const { return (size_t)tab_rows * tab_cols; }
  const Fe* tab_data() const { return table.empty() ? (const Fe*)tab_src : table.data(); }
  void keep_table() {
    if (tab_rows && table.empty()) table.assign((const Fe*)tab_src, (const Fe*)tab_src + tab_elems());
    tab_src = nullptr;
  }

  uint32_t n_inputs() const { return 1 + n_inv + n_carry + 2 * n_adv; }
  uint32_t in_j() const { return 0; }
  uint32_t in_inv(uint32_t k) const { return 1 + k; }
  uint32_t in_carry(uint32_t k) const { return 1 + n_inv + k; }
  uint32_t in_cur(uint32_t k) const { return 1 + n_inv + n_carry + k; }
  uint32_t in_next(uint32_t k) const { return 1 + n_inv + n_carry + n_adv + k; }
  bool same_body(const RoundRecord& o) const {
    return n_inv == o.n_inv && n_carry == o.n_carry && n_adv == o.n_adv && nodes == o.nodes && consts == o.consts && carry_out == o.carry_out &&
           tab_rows == o.tab_rows && tab_cols == o.tab_cols &&
           (tab_rows == 0 || tab_data() == o.tab_data() || memcmp(tab_data(), o.tab_data(), tab_elems() * sizeof(Fe)) == 0);
  }
  vdf_round_tape view() const {
    vdf_round_tape t;
    t.ops = ops.data(); t.n_ops = ops.size();
    t.consts = (const vdf_fe*)consts.data(); t.n_consts = consts.size();
    t.n_slots = n_slots; t.n_vars = n_vars; t.n_cons = n_cons; t.n_inv = n_inv; t.n_adv = n_adv;
    t.table = tab_rows ? (const vdf_fe*)tab_data() : nullptr; t.tab_rows = tab_rows; t.tab_cols = tab_cols;      // (host memory)
    return t;
  }
};

// the one vdf_cs_repeat of a custom circuit's synthesis, as the prover needs it afterwards
struct RepeatState {
  bool used = false;
  RoundRecord rec;
  uint64_t t = 0;
  size_t lanes = 1, lane_stride = 0;               // vdf_cs_repeat_lanes: chains side by side, lane l's advice lane_stride entries after lane l - 1's
  size_t var_begin = 0;                            // index of the first variable of repetition 0 in the witness
  size_t row_begin = 0;                            // ... and of its first constraint in the shape
  const void* d_advice = nullptr;                  // witness mode, advice in device memory: the variables were skipped (cs.dev_begin / dev_len);
                                                   // a probe: the advice pointer as the circuit handed it over, never read
  std::vector<Fe> inv;                             // ... and the values of inv (lanes * n_inv, lane-major), for the kernel
};

// Runs the body once on a recording handle; VDF_ERR_BAD_ARG (message through fail()) for a body that fails, uses a handle it does not
// own or exceeds a cap.  `is_witness`: what vdf_cs_is_witness answers inside the body.
int record_round_body(CS* cs, const vdf_round_body* b, RoundRecord* out);
// One repetition over cs with real calls.  carry: n_carry numbers, replaced by the repetition's carry_out.  cur / next: the advice
// entries' values (witness mode; carry values are overridden by cur), or null (shape mode).  scratch: reused between repetitions.
void replay_round(CS& cs, const RoundRecord& r, uint64_t j, const std::vector<Num>& inv, std::vector<Num>& carry, const Fe* cur, const Fe* next,
                  std::vector<Num>& scratch);
// the device program's semantics on the host (vdf_nova_round_tape_eval); checks every index like the launcher does
int eval_round_tape(int field, const vdf_round_tape* tape, uint64_t t, const Fe* inv, const Fe* advice, Fe* out);
// A walk body (vdf_nova.h vdf_walk_body) run once on a recording handle and compiled into a walk tape: the record has no carry, no
// variable and no constraint; its n_vars = n_adv columns are the handles the body left in cur_out.
// forward: the body is a forward body (vdf_nova_forward_body_record): the entry it is handed is entry j, loaded with ADV b = 0, and
// vdf_cs_pow and vdf_cs_pow_chain are legal.
int record_walk_body(CS* cs, const vdf_walk_body* b, RoundRecord* out, bool forward = false);
// vdf_round_tape_walk on the host (vdf_nova_walk_tape_eval): the same arguments, the same refusals, host memory
int eval_walk_tape(int field, const vdf_round_tape* tape, const Fe* inv, Fe* entries, size_t n, uint64_t rounds, Fe* trace, size_t walk_stride,
                   size_t top, size_t group, size_t group_stride, uint64_t j_base, uint64_t j_group_step, int heads, const Fe* expect, int32_t* ok);
// vdf_round_tape_run_lanes and vdf_round_tape_walk_lanes on the host (vdf_nova_round_tape_eval_lanes / vdf_nova_walk_tape_eval_lanes)
int eval_round_tape_lanes(int field, const vdf_round_tape* tape, uint64_t t, size_t lanes, const Fe* inv, const Fe* advice, size_t lane_stride,
                          Fe* out);
int eval_walk_tape_lanes(int field, const vdf_round_tape* tape, size_t lanes, const Fe* inv, Fe* entries, size_t n, uint64_t rounds, Fe* trace,
                         size_t walk_stride, size_t top, size_t group, size_t group_stride, const uint64_t* j_base, uint64_t j_group_step,
                         int heads, const Fe* expect, int32_t* ok);
// vdf_round_tape_forward_walk on the host (vdf_nova_forward_tape_eval): the same arguments, the same refusals, host memory
int eval_forward_tape(int field, const vdf_round_tape* tape, const Fe* inv, Fe* entries, size_t n, uint64_t rounds, Fe* checkpoints,
                      uint64_t every, size_t cp_stride, Fe* trace, size_t walk_stride, uint64_t base, uint64_t j_base, uint64_t j_walk_step);
// vdf_round_tape_rebuild_lanes on the host (vdf_nova_forward_tape_rebuild_eval_lanes): the same arguments, the same refusals, host memory
int eval_forward_tape_rebuild_lanes(int field, const vdf_round_tape* tape, size_t lanes, const Fe* inv, Fe* entries, size_t n, uint64_t rounds,
                                    Fe* trace, size_t walk_stride, uint64_t base, size_t group, size_t group_stride, const uint64_t* j_base,
                                    uint64_t j_group_step, int heads, const Fe* expect, int32_t* ok);
// "" where a tape's table names the same row for the round body's step-local j and for the chain-global J of what runs the tape over
// a chain (`whose`: "walk" or "forward" tape; `sees`: "walks'" or "evaluator's" J): tab_rows divides t and every lane's j_base
std::string tape_table_rows_fit_chain(const vdf_round_tape* tape, uint64_t t, size_t lanes, const uint64_t* j_base, const char* whose, const char* sees);

// The periodic rows of a repeat, as detect_periodic_rows read them off a shape's triples (include/vdf_hip.h vdf_periodic_rows):
// rows [row_begin, row_begin + row_count) are repetitions lead .. t - 1, and `view` is what the kernel and the host evaluator take.
struct PeriodicRows {
  bool valid = false;
  uint64_t lead = 0;
  size_t row_begin = 0, row_count = 0;
  uint32_t n_cons = 0, n_vars = 0;
  std::vector<uint16_t> row_start;
  std::vector<vdf_periodic_term> terms;
  std::vector<Fe> consts;
  vdf_periodic_rows view() const {
    vdf_periodic_rows v;
    v.n_cons = n_cons; v.n_vars = n_vars; v.j0 = lead;
    v.row_start = row_start.data();
    v.terms = terms.data(); v.n_terms = terms.size();
    v.consts = (const vdf_fe*)consts.data(); v.n_consts = consts.size();
    return v;
  }
};
// Are the rows of repetitions j0 .. t - 1 (n_cons each from row_begin on, the variables of repetition j at seg_begin + j n_vars)
// periodic, for the smallest j0 in 0 .. 4?  The pattern is taken from repetition j0, the slopes from j0 + 1, and then EVERY triple
// of EVERY repetition in all three matrices is compared with it.  false (and *out untouched): a mismatch anywhere, fewer than two
// periodic repetitions, a row of more than VDF_PERIODIC_MAX_ROW_TERMS terms, or a cap of the description exceeded.
bool detect_periodic_rows(const Coo m[3], const Field& F, size_t seg_begin, size_t n_vars, size_t row_begin, size_t n_cons, uint64_t t,
                          PeriodicRows* out);
// vdf_nifs_cross_term_periodic on the host (vdf_nova_periodic_rows_eval): the same arguments, the same refusals, host memory
int eval_periodic_rows(int field, const vdf_periodic_rows* rows, uint64_t j_first, uint64_t reps, size_t seg_begin, size_t row_begin,
                       size_t num_cols, size_t num_cons, const Fe* z2, const Fe* az1, const Fe* bz1, const Fe* cz1, const Fe* u1, Fe* az2,
                       Fe* bz2, Fe* cz2, Fe* T);
// a description into the caller's arrays of the caps, as the host-only entry points of vdf_nova.h hand it out
void periodic_rows_export(const PeriodicRows& pr, uint16_t* row_start, vdf_periodic_term* terms, vdf_fe* consts, vdf_periodic_rows* out,
                          uint64_t* lead, uint64_t* first_row, uint64_t* row_count);

}  // namespace vdfnova

// the handle a synthesize callback receives; `rec` set: the recording handle a round body receives (cs is then only asked for its mode)
struct vdf_cs {
  vdfnova::CS* cs = nullptr;
  std::vector<vdfnova::Num> pool;
  bool bad = false;
  vdfnova::RoundRecord* rec = nullptr;
  vdfnova::RepeatState* rep = nullptr;             // where a vdf_cs_repeat on this handle leaves its record (null: repeats are refused)
  vdf_ctx* ctx = nullptr;                          // for advice in device memory: the copy of its last entry (null: such advice is refused)
  uint32_t rec_calls = 0;
  bool walk = false;                               // the recording is a walk body's (vdf_nova_walk_body_record): value arithmetic only
  bool forward = false;                            // ... a forward body's (vdf_nova_forward_body_record): vdf_cs_pow / _pow_chain are legal
  const vdf_fe* step_advice = nullptr;             // vdf_cs_step_advice: the device trace of the step a custom chain drives (witness synthesis only)
  size_t step_advice_elems = 0;                    // ... and its length in elements: lanes * (t + 1) * n_adv of the parameters' repeat
  bool probe = false;                              // vdf_cs_is_probe: the extra synthesis of tuning.custom_ahead -- a vdf_cs_repeat records the body and
                                                   // keeps `inv`, reads no advice and makes no variable (rounds_host.cpp)
};
