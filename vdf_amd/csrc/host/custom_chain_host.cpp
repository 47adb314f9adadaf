// libvdf_nova.so, part 2c: the chain of a custom step circuit (vdf_custom_chain, include/vdf_nova.h) -- what circuits_host.cpp is
// to the built-in kinds: the checkpoints of a chain on the host, and per step a device trace rebuilt by the chain's walk tape
// (vdf_round_tape_walk; vdf_round_tape_walk_lanes for a chain of several lanes) on a side queue, a window ahead of the prover.
// An ASCENDING chain (rounds without a cheap inverse) rebuilds them by its forward tape instead (vdf_round_tape_rebuild_lanes): the
// two hooks that know a direction are stage_walks and launch; the window above them does not.
// A GROWING chain (vdf_nova_custom_chain_begin) gets its steps one push at a time, as checkpoints or as whole traces; a step pushed
// as a trace is "walked" by a job of no walks whose set-up uploads the host copy.
#include <atomic>
#include "nova_internal.hpp"
#include "../tape_launch.h"

using namespace vdfnova;

// The walks themselves are TraceWalks (trace_walks.hpp); the chain says what is walked: entries of n_adv elements, by its tape, over
// steps that are always a run [first, first + count), walk (li lanes + l) per + m being lane l's interval m of step first + li.
struct vdf_custom_chain final : WalkOwner {
  vdf_custom_chain() : WalkOwner("chain's", "steps") {}
  int field = VDF_FIELD_FQ;
  uint64_t t = 0, every = 0;
  size_t lanes = 1;                        // chains side by side in every step (vdf_cs_repeat_lanes)
  bool ascending = false;                  // the tape is the chain's forward tape: walks start below their interval and land above it
  uint64_t launch_bound = 0;               // ascending: the rounds one launch of the tape may run, min(1,024, the work cap / products)
  uint64_t launch_default = 0;             // what a job runs with when its caller asks for 0 (vdf_nova_custom_chain_set_launch_rounds)
  uint64_t launch_rounds_of(uint64_t asked) const {
    if (!asked) asked = launch_default;
    return !ascending ? asked : asked ? std::min(asked, launch_bound) : launch_bound;
  }
  std::vector<uint64_t> j_base;            // per lane
  size_t per = 0, na = 0;                  // walks per step AND LANE, elements per entry
  std::vector<vdf_tape_op> ops;
  std::vector<Fe> consts, inv;             // inv: lanes * n_inv
  std::vector<std::vector<Fe>> cp;         // per lane: (steps * per + 1) entries, forward order -- a lane of its own, so that it grows in
                                           // place; handed over as traces: the ONE entry the chain ends on
  // a growing chain: NONE until the first push decides; TRACES: adv[k] is step k's host copy (lanes * (t + 1) entries) until released
  enum Handover { CHECKPOINTS, NONE, TRACES } handover = CHECKPOINTS;
  bool growing = false;
  std::vector<std::vector<Fe>> adv;
  const Fe* end_of(size_t l) const { return cp[l].data() + cp[l].size() - na; }
  size_t cp_elems() const { size_t n = 0; for (const auto& l : cp) n += l.size(); return n; }
  size_t adv_elems() const { size_t n = 0; for (const auto& a : adv) n += a.size(); return n; }
  std::vector<Fe> table;                   // the walk tape's table (VDF_TAPE_TAB), a host copy ...
  std::atomic<void*> d_table{nullptr};     // ... and its ONE device copy, made by the first job on the traces' device, freed with the
                                           // chain; published only once it is whole (vdf_nova_custom_chain_memory may ask from another thread)
  std::vector<Fe> stage;                 // lanes > 1, while a job is pending: the walks' starts, then their targets, gathered
                                           // step-major, lane-minor (freed when the job resolves)
  std::vector<TraceSlot> v;
  vdf_round_tape tape;                     // into ops / consts
  TraceWalks walk{this};                   // (walk.home: where the traces live)

  TraceSlot& slot(size_t k) override { return v[k]; }
  void shape(size_t, WalkJob* j) override {
    j->every = handover == TRACES ? 0 : every;                  // traces handed over: no walks and no rounds, set-up uploads them
    j->launch_rounds = launch_rounds_of(j->launch_rounds);      // (set by the window before it asks for the shape)
    j->trace_bytes = lanes * (t + 1) * na * 32;
    j->step_walks = handover == TRACES ? 0 : lanes * per;
    j->entry_bytes = na * 32;
  }
  // walk li * per + m stands on the checkpoint above interval m of step lo + li and must land on the one below it: both runs
  // are contiguous in the lane's checkpoints; with more lanes than one they are gathered step-major, lane-minor (the walks'
  // order), into a staging vector that lives until the job resolves.  Ascending: the same two runs, the other way round.
  void stage_walks(const WalkJob& j, const void** starts, const void** expects) override {
    stage_descending(j, ascending ? expects : starts, ascending ? starts : expects);
  }
  void stage_descending(const WalkJob& j, const void** starts, const void** expects) {
    const size_t lo = j.steps[0];
    *expects = cp[0].data() + lo * per * na;
    *starts = cp[0].data() + lo * per * na + na;
    if (lanes == 1) return;
    const size_t run = per * na;
    stage.resize(2 * j.walks * na);
    for (size_t li = 0; li < j.steps.size(); ++li)
      for (size_t l = 0; l < lanes; ++l) {
        const Fe* src = cp[l].data() + (lo + li) * per * na;
        memcpy(stage.data() + (li * lanes + l) * run, src + na, run * 32);
        memcpy(stage.data() + j.walks * na + (li * lanes + l) * run, src, run * 32);
      }
    *starts = stage.data();
    *expects = stage.data() + j.walks * na;
  }
  void unstage() override { std::vector<Fe>().swap(stage); }
  // the table goes to the device once, on the queue the walks run on and in front of them; traces handed over are uploaded here,
  // step li's host copy into trace li of the job's block (materialize has refused a step whose copy is gone)
  int setup(vdf_ctx* q, const WalkJob& j, const WalkScratch&) override {
    if (handover == TRACES) {
      for (size_t li = 0; li < j.steps.size(); ++li) {
        const int rc = vdf_dev_memcpy(q, (char*)j.block->d + li * j.trace_bytes, adv[j.steps[li]].data(), j.trace_bytes);
        if (rc != VDF_OK) return rc;
      }
      return VDF_OK;
    }
    if (table.empty() || d_table.load()) return VDF_OK;
    void* d = nullptr;
    int rc = vdf_dev_alloc(walk.home, table.size() * 32, &d);
    if (rc != VDF_OK) return rc;
    rc = vdf_dev_memcpy(q, d, table.data(), table.size() * 32);
    if (rc != VDF_OK) { vdf_dev_free(walk.home, d); return rc; }      // nothing is kept: the next job tries again
    tape.table = (const vdf_fe*)d;
    d_table.store(d);
    return VDF_OK;
  }
  // the comparison rides in the last slice
  int launch(vdf_ctx* q, const WalkJob& j, const WalkScratch& s, uint64_t rounds, uint64_t top, int last) override {
    uint64_t jb[VDF_TAPE_MAX_LANES];
    for (size_t l = 0; l < lanes; ++l) jb[l] = j_base[l] + (uint64_t)j.steps[0] * t;
    if (ascending)                                   // top = every - done (walk_slice): the rounds behind the walks are every - top
      HIPCALL(q, vdf_round_tape_rebuild_lanes(q, field, &tape, lanes, (const vdf_fe*)inv.data(), (vdf_fe*)s.d_walk, j.walks, rounds, (vdf_fe*)j.block->d,
                                              (size_t)every, every - top, per, (size_t)(t + 1), jb, t, 1, last ? (const vdf_fe*)s.d_expect : nullptr,
                                              last ? s.h_ok : nullptr));
    else if (lanes == 1)
      HIPCALL(q, vdf_round_tape_walk(q, field, &tape, (const vdf_fe*)inv.data(), (vdf_fe*)s.d_walk, j.walks, rounds, (vdf_fe*)j.block->d, (size_t)every,
                                     (size_t)top, per, (size_t)(t + 1), jb[0], t, last, last ? (const vdf_fe*)s.d_expect : nullptr, last ? s.h_ok : nullptr));
    else                                             // every lane of every step of the window in ONE launch: group G = step * lanes + lane
      HIPCALL(q, vdf_round_tape_walk_lanes(q, field, &tape, lanes, (const vdf_fe*)inv.data(), (vdf_fe*)s.d_walk, j.walks, rounds, (vdf_fe*)j.block->d,
                                           (size_t)every, (size_t)top, per, (size_t)(t + 1), jb, t, last, last ? (const vdf_fe*)s.d_expect : nullptr,
                                           last ? s.h_ok : nullptr));
    return VDF_OK;
  }
  std::string missed(size_t k, size_t walk) override {
    return "step " + std::to_string(k) + (lanes > 1 ? ", lane " + std::to_string(walk / per) : std::string()) + ": a walk did not land on the checkpoint " + (ascending ? "above" : "below") + " it";
  }
};

namespace vdfnova {
ChainInfo chain_info(const vdf_custom_chain* c) { return ChainInfo{c->field, c->t, c->na, c->v.size(), c->walk.home, c->lanes}; }
TraceWalks& chain_walks(vdf_custom_chain* c) { return c->walk; }
int chain_need(vdf_custom_chain* c, size_t k, const vdf_fe** d_trace) {
  if (c->walk.covers(k)) { int rc = c->walk.resolve(nullptr, 0, 0); if (rc != VDF_OK) return rc; }
  if (!c->v[k].d_trace) return fail(VDF_ERR_BAD_ARG, "advice of step " + std::to_string(k) + " not materialised");
  *d_trace = (const vdf_fe*)c->v[k].d_trace;
  return VDF_OK;
}
// the pending walks are wanted by the step that proves their first step
int chain_pump(vdf_custom_chain* c, size_t k) { return c->walk.pump(k, 0); }
const vdf_fe* chain_ready(const vdf_custom_chain* c, size_t k) {
  return k < c->v.size() && !c->walk.covers(k) ? (const vdf_fe*)c->v[k].d_trace : nullptr;
}
}  // namespace vdfnova

namespace vdfnova {
std::string tape_table_rows_fit_chain(const vdf_round_tape* tape, uint64_t t, size_t lanes, const uint64_t* j_base, const char* whose, const char* sees) {
  if (tape->tab_rows == 0) return "";
  const std::string head = std::string("the ") + whose + " tape's tab_rows must divide ", tail = std::string(" (the round body's j is step-local, the ") + sees + " J chain-global)";
  if (t % tape->tab_rows != 0) return head + "t" + tail;
  for (size_t l = 0; l < lanes; ++l)
    if (j_base[l] % tape->tab_rows != 0) return head + "every j_base" + tail;
  return "";
}
}  // namespace vdfnova

extern "C" {
int vdf_nova_custom_chain_slice(uint64_t every, uint64_t launch_rounds, uint64_t done, uint64_t budget, uint64_t* rounds, uint64_t* top,
                                int* last) {
  if (!rounds || !top || !last) return fail(VDF_ERR_BAD_ARG, "null argument");
  if (every == 0 || done >= every) return fail(VDF_ERR_BAD_ARG, "`every` must be positive and `done` below it");
  walk_slice(every, launch_rounds, done, budget, rounds, top, last);
  return VDF_OK;
}
// one chain's checkpoints: the stride of a single lane (refused by the constructor otherwise)
static size_t single_stride(uint64_t t, uint64_t every, size_t num_steps) {
  return every && t && num_steps <= ((size_t)1 << 40) ? num_steps * (size_t)(t / every) + 1 : 1;
}
// all four constructors and vdf_nova_custom_chain_begin: `walk_tape` is the chain's walk tape, or (ascending) its forward tape.
// growing: no steps yet, `checkpoints` is entry 0 of every lane (lane_stride 1) and every / num_steps are the pushes' to say.
static int chain_from_checkpoints(int fid, const vdf_round_tape* walk_tape, bool ascending, const vdf_fe* inv, uint64_t t, uint64_t every,
                                  size_t num_steps, size_t lanes, const vdf_fe* checkpoints, size_t lane_stride, const uint64_t* j_base,
                                  vdf_custom_chain** out, bool growing = false) {
  return nova_guard([&]() -> int {
    if (!out) return fail(VDF_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
    if (!walk_tape || !checkpoints || !j_base) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (!growing && num_steps == 0) return fail(VDF_ERR_BAD_ARG, "num_steps must be > 0");
    if (t == 0 || t >= (1ull << 31)) return fail(VDF_ERR_BAD_ARG, "t out of range (1 <= t < 2^31, vdf_cs_repeat)");
    if (!growing && (every == 0 || t % every != 0)) return fail(VDF_ERR_BAD_ARG, "`every` must be positive and divide t");
    if (lanes == 0 || lanes > VDF_TAPE_MAX_LANES) return fail(VDF_ERR_BAD_ARG, "lanes must be 1 .. VDF_TAPE_MAX_LANES");
    // the check the walk's launcher applies, by its host restatement with nothing to walk (a null `inv` the tape reads included):
    // vdf_round_tape_walk's for one lane, vdf_round_tape_walk_lanes' (lanes * n_inv, n_inv more slots) for more
    if (ascending) {                                   // vdf_round_tape_rebuild_lanes', for any lanes
      const int rc = eval_forward_tape_rebuild_lanes(fid, walk_tape, lanes, (const Fe*)inv, nullptr, 0, 0, nullptr, 0, 0, 0, 0, j_base, 0, 0, nullptr, nullptr);
      if (rc != VDF_OK) return rc;
    } else {
      const int rc = lanes == 1 ? eval_walk_tape(fid, walk_tape, (const Fe*)inv, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, 0, nullptr, nullptr)
                                : eval_walk_tape_lanes(fid, walk_tape, lanes, (const Fe*)inv, nullptr, 0, 0, nullptr, 0, 0, 0, 0, j_base, 0, 0, nullptr, nullptr);
      if (rc != VDF_OK) return rc;
    }
    // a chain's walks see the chain-global J (step g's walks j_base + g * t + ...), the round body's j is step-local: the two name
    // the same row of a table only when its rows divide t and every j_base
    const std::string rows = tape_table_rows_fit_chain(walk_tape, t, lanes, j_base, "walk", "walks'");
    if (!rows.empty()) return fail(VDF_ERR_BAD_ARG, rows);
    const size_t per = growing ? 0 : (size_t)(t / every), na = walk_tape->n_adv;
    if (!growing && num_steps > ((size_t)1 << 40) / per) return fail(VDF_ERR_BAD_LENGTH, "too many checkpoints");
    const size_t entries = num_steps * per + 1;
    if (lane_stride < entries || lane_stride > ((size_t)1 << 44)) return fail(VDF_ERR_BAD_ARG, "lane_stride must be at least num_steps * (t / every) + 1");
    std::unique_ptr<vdf_custom_chain> c(new vdf_custom_chain());
    c->field = fid; c->t = t; c->every = every; c->lanes = lanes; c->per = per; c->na = na;
    c->ascending = ascending;
    c->growing = growing;
    if (growing) c->handover = vdf_custom_chain::NONE;
    if (ascending) c->launch_bound = vdflaunch::forward_launch_bound(walk_tape);
    c->j_base.assign(j_base, j_base + lanes);
    c->ops.assign(walk_tape->ops, walk_tape->ops + walk_tape->n_ops);
    c->consts.assign((const Fe*)walk_tape->consts, (const Fe*)walk_tape->consts + walk_tape->n_consts);
    if (walk_tape->n_inv) c->inv.assign((const Fe*)inv, (const Fe*)inv + lanes * walk_tape->n_inv);
    c->tape = *walk_tape;
    c->tape.ops = c->ops.data();
    c->tape.consts = (const vdf_fe*)c->consts.data();
    if (walk_tape->tab_rows) c->table.assign((const Fe*)walk_tape->table, (const Fe*)walk_tape->table + (size_t)walk_tape->tab_rows * walk_tape->tab_cols);
    c->tape.table = nullptr;                           // the device copy, once a job has made it (setup)
    c->cp.resize(lanes);
    const bool device = vdf_ptr_is_device(checkpoints);
    for (size_t l = 0; l < lanes; ++l) {
      const Fe* src = (const Fe*)checkpoints + l * lane_stride * na;
      c->cp[l].resize(entries * na);
      if (device) {
        // (a copy only, after every refusal: the runtime finds the pointer's device, nothing is allocated there)
        const int rc = vdf_ptr_download(c->cp[l].data(), src, entries * na * 32);
        if (rc != VDF_OK) return fail(rc, std::string("checkpoints: ") + vdf_last_error(nullptr));
      } else memcpy(c->cp[l].data(), src, entries * na * 32);
    }
    c->v.resize(num_steps);
    *out = c.release();
    return VDF_OK;
  });
}
int vdf_nova_custom_chain_from_checkpoints(int fid, const vdf_round_tape* walk_tape, const vdf_fe* inv, uint64_t t, uint64_t every,
                                           size_t num_steps, const vdf_fe* checkpoints, uint64_t j_base, vdf_custom_chain** out) {
  return chain_from_checkpoints(fid, walk_tape, false, inv, t, every, num_steps, 1, checkpoints, single_stride(t, every, num_steps), &j_base, out);
}
int vdf_nova_custom_chain_lanes_from_checkpoints(int fid, const vdf_round_tape* walk_tape, const vdf_fe* inv, uint64_t t, uint64_t every,
                                                 size_t num_steps, size_t lanes, const vdf_fe* checkpoints, size_t lane_stride,
                                                 const uint64_t* j_base, vdf_custom_chain** out) {
  return chain_from_checkpoints(fid, walk_tape, false, inv, t, every, num_steps, lanes, checkpoints, lane_stride, j_base, out);
}
int vdf_nova_custom_chain_from_checkpoints_forward(int fid, const vdf_round_tape* forward_tape, const vdf_fe* inv, uint64_t t, uint64_t every,
                                                   size_t num_steps, const vdf_fe* checkpoints, uint64_t j_base, vdf_custom_chain** out) {
  return chain_from_checkpoints(fid, forward_tape, true, inv, t, every, num_steps, 1, checkpoints, single_stride(t, every, num_steps), &j_base, out);
}
int vdf_nova_custom_chain_lanes_from_checkpoints_forward(int fid, const vdf_round_tape* forward_tape, const vdf_fe* inv, uint64_t t,
                                                         uint64_t every, size_t num_steps, size_t lanes, const vdf_fe* checkpoints,
                                                         size_t lane_stride, const uint64_t* j_base, vdf_custom_chain** out) {
  return chain_from_checkpoints(fid, forward_tape, true, inv, t, every, num_steps, lanes, checkpoints, lane_stride, j_base, out);
}
int vdf_nova_custom_chain_begin(int fid, const vdf_round_tape* tape, int direction, const vdf_fe* inv, uint64_t t, size_t lanes,
                                const vdf_fe* initial, const uint64_t* j_base, vdf_custom_chain** out) {
  if (direction != VDF_CHAIN_DESCENDING && direction != VDF_CHAIN_ASCENDING) {
    if (out) *out = nullptr;
    return fail(VDF_ERR_BAD_ARG, "direction must be VDF_CHAIN_DESCENDING or VDF_CHAIN_ASCENDING");
  }
  return chain_from_checkpoints(fid, tape, direction == VDF_CHAIN_ASCENDING, inv, t, 0, 0, lanes, initial, 1, j_base, out, true);
}
// One more step of a growing chain.  entries: what a lane hands over, per + 1 checkpoints or t + 1 trace entries; lane l's run starts
// lane_stride entries after lane l - 1's (not read for one lane).  Nothing is appended unless every lane starts on the chain's end.
static int chain_push(vdf_custom_chain* c, vdf_custom_chain::Handover kind, uint64_t every, const vdf_fe* src, size_t lane_stride) {
  return nova_guard([&]() -> int {
    if (!c || !src) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (!c->growing) return fail(VDF_ERR_BAD_ARG, "the chain was made whole from its checkpoints: only a chain of vdf_nova_custom_chain_begin grows");
    const bool traces = kind == vdf_custom_chain::TRACES;
    if (c->handover != vdf_custom_chain::NONE && c->handover != kind)
      return fail(VDF_ERR_BAD_ARG, std::string("the chain's steps are handed over as ") + (traces ? "checkpoints" : "whole traces") + ": one hand-over per chain");
    if (!traces) {
      if (every == 0 || c->t % every != 0) return fail(VDF_ERR_BAD_ARG, "`every` must be positive and divide t");
      if (c->handover != vdf_custom_chain::NONE && every != c->every)
        return fail(VDF_ERR_BAD_ARG, "every = " + std::to_string(every) + ", the chain's first push said " + std::to_string(c->every));
    }
    const size_t na = c->na, per = traces ? 0 : (size_t)(c->t / every), entries = traces ? (size_t)c->t + 1 : per + 1;
    if (c->lanes > 1 && (lane_stride < entries || lane_stride > ((size_t)1 << 44)))
      return fail(VDF_ERR_BAD_ARG, std::string("lane_stride must be at least ") + (traces ? "t + 1" : "t / every + 1"));
    if (!traces && c->v.size() + 1 > ((size_t)1 << 40) / per) return fail(VDF_ERR_BAD_LENGTH, "too many checkpoints");
    const bool device = vdf_ptr_is_device(src);
    if (traces && device) return fail(VDF_ERR_BAD_ARG, "advice: host memory expected");
    std::vector<Fe> got(c->lanes * entries * na);
    for (size_t l = 0; l < c->lanes; ++l) {
      const Fe* from = (const Fe*)src + l * lane_stride * na;
      if (device) {
        const int rc = vdf_ptr_download(got.data() + l * entries * na, from, entries * na * 32);
        if (rc != VDF_OK) return fail(rc, std::string("checkpoints: ") + vdf_last_error(nullptr));
      } else memcpy(got.data() + l * entries * na, from, entries * na * 32);
    }
    for (size_t l = 0; l < c->lanes; ++l)
      if (memcmp(got.data() + l * entries * na, c->end_of(l), na * 32) != 0)
        return fail(VDF_ERR_BAD_ARG, "lane " + std::to_string(l) + ": the step does not start on the chain's end");
    // from here nothing is refused; room first, so that a failed allocation leaves the chain as it was
    c->v.reserve(c->v.size() + 1);
    if (traces) c->adv.reserve(c->adv.size() + 1);
    else for (size_t l = 0; l < c->lanes; ++l) c->cp[l].reserve(c->cp[l].size() + per * na);
    for (size_t l = 0; l < c->lanes; ++l) {
      const Fe* lane = got.data() + l * entries * na;
      if (traces) memcpy(c->cp[l].data(), lane + (size_t)c->t * na, na * 32);      // the chain's new end
      else c->cp[l].insert(c->cp[l].end(), lane + na, lane + entries * na);
    }
    if (traces) c->adv.push_back(std::move(got));
    else { c->every = every; c->per = per; }
    c->handover = kind;
    c->v.emplace_back();
    return VDF_OK;
  });
}
int vdf_nova_custom_chain_push_checkpoints(vdf_custom_chain* c, uint64_t every, const vdf_fe* checkpoints, size_t lane_stride) {
  return chain_push(c, vdf_custom_chain::CHECKPOINTS, every, checkpoints, lane_stride);
}
int vdf_nova_custom_chain_push_advice(vdf_custom_chain* c, const vdf_fe* advice, size_t lane_stride) {
  return chain_push(c, vdf_custom_chain::TRACES, 0, advice, lane_stride);
}
int vdf_nova_custom_chain_direction(const vdf_custom_chain* c) { return !c ? -1 : c->ascending ? VDF_CHAIN_ASCENDING : VDF_CHAIN_DESCENDING; }
int vdf_nova_custom_chain_launch_rounds(const vdf_custom_chain* c, uint64_t launch_rounds, uint64_t* out) {
  if (!c || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
  *out = c->launch_rounds_of(launch_rounds);
  return VDF_OK;
}
int vdf_nova_custom_chain_set_launch_rounds(vdf_custom_chain* c, uint64_t launch_rounds) {
  if (!c) return fail(VDF_ERR_BAD_ARG, "null argument");
  c->launch_default = launch_rounds;
  return VDF_OK;
}
int vdf_nova_custom_chain_materialize(vdf_ctx* ctx, vdf_custom_chain* c, size_t first, size_t count, int wait, uint64_t launch_rounds,
                                      int* bad) {
  return nova_guard([&]() -> int {
    if (!ctx || !c) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (first > c->v.size() || count > c->v.size() - first) return fail(VDF_ERR_BAD_LENGTH, "step range out of bounds");
    if (bad) for (size_t k = 0; k < count; ++k) bad[k] = 0;
    const int pending = c->walk.resolve(bad, first, count);             // one job at a time; its verdict is this call's too
    if (pending != VDF_OK && pending != VDF_ERR_BAD_ARG) return pending;
    // the steps of the range without a trace, from the first to the last of them (a resident step between two of them is walked again)
    size_t lo = first + count, hi = first;
    for (size_t k = first; k < first + count; ++k) if (!c->v[k].d_trace) { lo = std::min(lo, k); hi = k + 1; }
    std::vector<size_t> steps;
    for (size_t k = lo; k < hi; ++k) steps.push_back(k);
    if (c->handover == vdf_custom_chain::TRACES)
      for (size_t k : steps)
        if (c->adv[k].empty()) return fail(VDF_ERR_BAD_ARG, "step " + std::to_string(k) + " was released: a growing chain does not keep the advice of a released step");
    if (steps.size() * c->lanes * c->per > ((size_t)1 << 31)) return fail(VDF_ERR_BAD_LENGTH, "more than 2^31 walks in a window");
    return c->walk.begin(ctx, std::move(steps), wait, launch_rounds, pending, bad, first, count);
  });
}
int vdf_nova_custom_chain_release(vdf_custom_chain* c, size_t first, size_t count) {
  return nova_guard([&]() -> int {
    if (!c) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (first > c->v.size() || count > c->v.size() - first) return fail(VDF_ERR_BAD_LENGTH, "step range out of bounds");
    const int pending = c->walk.covers(first, count) ? c->walk.resolve(nullptr, 0, 0) : VDF_OK;
    c->walk.release(first, count, false);
    if (c->handover == vdf_custom_chain::TRACES)                        // a long stream holds a bounded number of traces
      for (size_t k = first; k < first + count; ++k) std::vector<Fe>().swap(c->adv[k]);
    return pending;
  });
}
int vdf_nova_custom_chain_memory(const vdf_custom_chain* c, size_t* resident_steps, uint64_t* device_bytes) {
  if (!c) return fail(VDF_ERR_BAD_ARG, "null argument");
  c->walk.memory(c->v.size(), resident_steps, device_bytes);
  if (device_bytes && c->d_table.load()) *device_bytes += c->table.size() * 32;      // the table's device copy
  return VDF_OK;
}
int vdf_nova_custom_chain_host_bytes(const vdf_custom_chain* c, uint64_t* bytes) {
  if (!c || !bytes) return fail(VDF_ERR_BAD_ARG, "null argument");
  *bytes = c->ops.size() * sizeof(vdf_tape_op) + (c->consts.size() + c->inv.size() + c->cp_elems() + c->adv_elems() + c->stage.size() + c->table.size()) * 32;
  return VDF_OK;
}
size_t vdf_nova_custom_chain_len(const vdf_custom_chain* c) { return c ? c->v.size() : 0; }
int vdf_nova_custom_chain_advice(vdf_custom_chain* c, size_t k, const vdf_fe** d_advice) {
  return nova_guard([&]() -> int {
    if (!c || !d_advice) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (k >= c->v.size()) return fail(VDF_ERR_BAD_LENGTH, "step index out of range");
    *d_advice = nullptr;
    if (c->walk.covers(k)) { int rc = c->walk.resolve(nullptr, 0, 0); if (rc != VDF_OK && rc != VDF_ERR_BAD_ARG) return rc; }
    *d_advice = (const vdf_fe*)c->v[k].d_trace;
    return VDF_OK;
  });
}
void vdf_nova_custom_chain_free(vdf_custom_chain* c) {
  if (!c) return;
  vdf_ctx* home = c->walk.home;
  c->walk.teardown(c->v.size());                       // (synchronises the walks' queue)
  if (c->d_table.load()) vdf_dev_free(home, c->d_table.load());
  delete c;
}
}  // extern "C"
