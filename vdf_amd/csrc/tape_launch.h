// What a launch of a tape is refused for beyond the tape's own rules (tape_rules.h), how many slots of LDS it takes, and -- for the
// ascending walks in groups (include/vdf_hip.h vdf_round_tape_rebuild_lanes) -- where walk w of a call stands: stated ONCE,
// header-only, as tape_rules.h states the rules of a tape.  libvdf_hip.so's launchers (rounds.hip, abi.hip) and libvdf_nova.so's host
// restatements (host/rounds_host.cpp) both read it, since neither library can call the other's internals: a call one side refuses
// the other refuses, with the same code and the same words, whichever faults it has.  The refusals are host code; the rebuild's
// index arithmetic is plain integer code compiled for the host and for the device (its kernel reads it too).  Where pointers must
// live, and which of the vectors may be null, is each caller's own check.
#pragma once
#include "tape_rules.h"

#if defined(__HIPCC__)
#define VDF_LAUNCH_FN __host__ __device__ inline
#else
#define VDF_LAUNCH_FN inline
#endif

namespace vdflaunch {

// ---- the ascending rebuild's index arithmetic ---------------------------------------------------------------------------------
// Walk w of a call: group G = w / group = g * lanes + l is lane l of step g (the groups of vdf_round_tape_walk_lanes), and before
// round 0 of the call the walk stands on local index k of its group's trace.  group != 0 (normalised by groups()).
struct Place {
  uint64_t G, g, k;
  uint32_t l;
  bool first;              // the first walk of its group: the one that writes the head
};
// group = 0: every walk is group 0, lane 0 of step 0 (every launch kind with groups normalises through here)
VDF_LAUNCH_FN void groups(uint64_t n, uint64_t* group, uint64_t* group_stride) {
  if (*group == 0) { *group = n; *group_stride = 0; }
}
VDF_LAUNCH_FN Place place(uint64_t w, uint64_t group, uint64_t walk_stride, uint64_t base, uint32_t lanes) {
  Place p;
  const uint64_t m = w % group;
  p.G = w / group;
  p.g = p.G / lanes;
  p.l = (uint32_t)(p.G % lanes);
  p.k = m * walk_stride + base;
  p.first = m == 0;
  return p;
}
// VDF_TAPE_J of the round a walk runs while it stands on local index k (modulo 2^64): the index of that entry, the j of the round
// body's repetition j, and the value the descending walk sees when it produces that entry.  lane_j_base: j_base[p.l]
VDF_LAUNCH_FN uint64_t counter(const Place& p, uint64_t lane_j_base, uint64_t j_group_step) { return lane_j_base + p.g * j_group_step + p.k; }
// the ENTRY of `trace` that holds local index k of the walk's group; a round run on k writes k + 1
VDF_LAUNCH_FN uint64_t trace_entry(const Place& p, uint64_t group_stride, uint64_t k) { return p.G * group_stride + k; }

// ---- the launch kinds -----------------------------------------------------------------------------------------------------------
// RUN, RUN_LANES: vdf_round_tape_run(_lanes); WALK, WALK_LANES: vdf_round_tape_walk(_lanes), descending; FORWARD:
// vdf_round_tape_forward_walk; REBUILD: vdf_round_tape_rebuild_lanes, ascending in groups and lanes
enum Kind { RUN, RUN_LANES, WALK, WALK_LANES, FORWARD, REBUILD };
inline vdftape::Mode mode_of(Kind k) { return k <= RUN_LANES ? vdftape::ROUND : k <= WALK_LANES ? vdftape::WALK : vdftape::FORWARD; }
inline bool in_lanes(Kind k) { return k == RUN_LANES || k == WALK_LANES || k == REBUILD; }

// The slots of LDS a lane of the launch keeps: the value file; the two entries of a walk; a lane's invariants where the lane is a
// per-thread value; the temporaries of a forward tape's chains.  The cap below and the launcher's dynamic LDS both read this.
inline uint32_t slots(Kind k, const vdf_round_tape* tp, const vdftape::Info& ti) {
  uint32_t s = tp->n_slots;
  if (k >= WALK) s += 2 * tp->n_adv;
  if (k == WALK_LANES || k == REBUILD) s += tp->n_inv;
  if (k == FORWARD || k == REBUILD) s += ti.chain_tmp;
  return s;
}
// [slot][half][lane] of 16-byte halves for the 64 lanes of a wavefront
inline size_t lds_bytes(Kind k, const vdf_round_tape* tp, const vdftape::Info& ti) { return (size_t)slots(k, tp, ti) * 2 * 64 * 16; }

// the rounds one launch of a forward tape runs when the caller names no number: 1,024 or what the work cap leaves
inline uint64_t forward_launch_bound(const vdftape::Info& ti) {
  const uint64_t cap = VDF_FORWARD_TAPE_MAX_WORK / ti.products;
  return cap < 1024 ? cap : 1024;
}
// ... of a tape as it stands; 0 for a tape FORWARD's rules refuse
inline uint64_t forward_launch_bound(const vdf_round_tape* tp) {
  vdftape::Info ti;
  return vdftape::check(tp, vdftape::FORWARD, &ti).empty() ? forward_launch_bound(ti) : 0;
}

// ---- the refusals -----------------------------------------------------------------------------------------------------------------
// code = VDF_OK: go on -- unless `nothing`: n = 0 or rounds = 0, the call is over and has done nothing.  ti: what tape_rules.h found
// out about the tape (filled once its rules have passed)
struct Verdict {
  int code = VDF_OK;
  std::string why;
  bool nothing = false;
  vdftape::Info ti = {1, 0, false};
  bool refused() const { return code != VDF_OK; }
};
inline Verdict refuse(int code, std::string why) { Verdict v; v.code = code; v.why = std::move(why); return v; }

inline Verdict t_range(uint64_t t) { return t == 0 || t >= (1ull << 31) ? refuse(VDF_ERR_BAD_LENGTH, "t out of range") : Verdict(); }

// rules 1 - 4 of every launch: the tape in the kind's mode, then what only a launch has -- the lanes, whose lanes * n_inv
// invariants (lane-major) all go into the argument block of VDF_TAPE_MAX_INV
inline Verdict tape_and_lanes(Kind kind, const vdf_round_tape* tp, size_t lanes, const vdf_fe* inv) {
  Verdict v;
  const std::string why = vdftape::check(tp, mode_of(kind), &v.ti);
  if (!why.empty()) return refuse(VDF_ERR_BAD_ARG, why);
  if (lanes == 0 || lanes > VDF_TAPE_MAX_LANES) return refuse(VDF_ERR_BAD_ARG, "lanes must be 1 .. VDF_TAPE_MAX_LANES");
  if (lanes * tp->n_inv > VDF_TAPE_MAX_INV) return refuse(VDF_ERR_BAD_ARG, "lanes * n_inv > VDF_TAPE_MAX_INV (all lanes' inv travel in the kernel arguments)");
  if (tp->n_inv && !inv) return refuse(VDF_ERR_BAD_ARG, "null inv");
  return v;
}

// vdf_round_tape_run (kind RUN: lanes = 1, lane_stride unread) and vdf_round_tape_run_lanes
inline Verdict round_launch(Kind kind, const vdf_round_tape* tp, uint64_t t, size_t lanes, const vdf_fe* inv, size_t lane_stride) {
  Verdict v = t_range(t);
  if (v.refused()) return v;
  v = tape_and_lanes(kind, tp, lanes, inv);
  if (v.refused()) return v;
  if (kind == RUN_LANES && (lane_stride < t + 1 || lane_stride > ((size_t)1 << 40))) return refuse(VDF_ERR_BAD_ARG, "lane_stride must be at least t + 1");
  return v;
}

// What the refusals of a walk look at.  lanes = 1 and j_base unread outside the lanes kinds; stand: `top` descending, `base`
// ascending; checkpoints / every: FORWARD's; trace, walk_stride, group, heads, expect, ok: unread by FORWARD.
struct Walk {
  Kind kind; const vdf_round_tape* tape; size_t lanes; const vdf_fe* inv; const uint64_t* j_base;
  size_t n; uint64_t rounds; const void *entries, *trace; uint64_t walk_stride, stand, group; int heads;
  const void* expect; const int32_t* ok; const void* checkpoints; uint64_t every;
};

inline Verdict walk_launch(const Walk& c) {
  const vdf_round_tape* tp = c.tape;
  const Kind k = c.kind;
  Verdict v = tape_and_lanes(k, tp, c.lanes, c.inv);
  if (v.refused()) return v;
  if (in_lanes(k) && !c.j_base) return refuse(VDF_ERR_BAD_ARG, "null j_base");
  static const char* const sum[] = {"walk tape: n_slots + 2 * n_adv", "walk tape in lanes: n_slots + 2 * n_adv + n_inv",
                                   "forward walk tape: n_slots + 2 * n_adv + the chains' n_tmp", "rebuild tape: n_slots + 2 * n_adv + n_inv + the chains' n_tmp"};
  if (slots(k, tp, v.ti) > VDF_WALK_MAX_SLOTS) return refuse(VDF_ERR_BAD_ARG, std::string(sum[k - WALK]) + " > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)");
  const bool descending = mode_of(k) == vdftape::WALK;
  if (c.rounds > (descending ? VDF_WALK_MAX_WORK : VDF_FORWARD_TAPE_MAX_WORK) / v.ti.products)
    return refuse(VDF_ERR_BAD_ARG, std::string("rounds x products per round > ") + (descending ? "VDF_WALK_MAX_WORK" : "VDF_FORWARD_TAPE_MAX_WORK") +
                                       " in one call: cut the walk");
  if (k == FORWARD ? c.checkpoints && c.every == 0 : c.expect && !c.ok)
    return refuse(VDF_ERR_BAD_ARG, k == FORWARD ? "checkpoints without `every`" : "expect without ok");
  if (c.n == 0 || c.rounds == 0) { v.nothing = true; return v; }
  if (c.n > ((size_t)1 << 31)) return refuse(k == REBUILD ? VDF_ERR_BAD_ARG : VDF_ERR_BAD_LENGTH, "more than 2^31 walks");
  if (!c.entries) return refuse(VDF_ERR_BAD_ARG, "null entries");
  // the kind's own geometry: a walk that writes a trace stays inside its run
  if (descending && c.trace) {
    if (c.stand + 1 < c.rounds) return refuse(VDF_ERR_BAD_ARG, "top < rounds - 1: the walk would write below its run");
    if (c.heads && c.stand < c.rounds) return refuse(VDF_ERR_BAD_ARG, "heads with top < rounds: the landing would be written below the run");
  }
  uint64_t group = c.group, group_stride = 0;
  groups(c.n, &group, &group_stride);
  if (k == REBUILD && c.trace && group > 1 && (c.stand > c.walk_stride || c.rounds > c.walk_stride - c.stand))
    return refuse(VDF_ERR_BAD_ARG, "base + rounds > walk_stride: the walk would write into the run of the walk above it");
  return v;
}

}  // namespace vdflaunch
