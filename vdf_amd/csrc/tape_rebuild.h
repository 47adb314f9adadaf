// Ascending walks in groups (include/vdf_hip.h vdf_round_tape_rebuild_lanes): where walk w of a call stands, which lane and step it
// belongs to, which counter it sees and where its trace lies -- and what a call is refused for beyond the tape's own rules --
// stated ONCE, header-only, as tape_rules.h states the rules of a tape: the kernel and the launcher (rounds.hip) and libvdf_nova.so's
// host restatement (host/rounds_host.cpp) all read the index arithmetic from here, since neither library can call the other's
// internals.  The arithmetic is plain integer code, compiled for the host and for the device; the refusals are host code.
#pragma once
#include "tape_rules.h"

#if defined(__HIPCC__)
#define VDF_REBUILD_FN __host__ __device__ inline
#else
#define VDF_REBUILD_FN inline
#endif

namespace vdfrebuild {

// Walk w of a call: group G = w / group = g * lanes + l is lane l of step g (the groups of vdf_round_tape_walk_lanes), and before
// round 0 of the call the walk stands on local index k of its group's trace.  group != 0 (normalised by groups()).
struct Place {
  uint64_t G, g, k;
  uint32_t l;
  bool first;              // the first walk of its group: the one that writes the head
};
// group = 0: every walk is group 0, lane 0 of step 0
VDF_REBUILD_FN void groups(uint64_t n, uint64_t* group, uint64_t* group_stride) {
  if (*group == 0) { *group = n; *group_stride = 0; }
}
VDF_REBUILD_FN Place place(uint64_t w, uint64_t group, uint64_t walk_stride, uint64_t base, uint32_t lanes) {
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
VDF_REBUILD_FN uint64_t counter(const Place& p, uint64_t lane_j_base, uint64_t j_group_step) { return lane_j_base + p.g * j_group_step + p.k; }
// the ENTRY of `trace` that holds local index k of the walk's group; a round run on k writes k + 1
VDF_REBUILD_FN uint64_t trace_entry(const Place& p, uint64_t group_stride, uint64_t k) { return p.G * group_stride + k; }

// What a call is refused for after vdftape::check(tape, FORWARD, &ti) has passed, in the order the launcher and the restatement
// both apply: "" to go on.  *nothing: n = 0 or rounds = 0, nothing to do.  (Where the pointers must live is each caller's own check.)
inline std::string refuse(const vdf_round_tape* tp, const vdftape::Info& ti, size_t lanes, const vdf_fe* inv, const uint64_t* j_base, size_t n,
                          uint64_t rounds, const void* entries, const void* trace, size_t walk_stride, uint64_t base, size_t group,
                          const void* expect, const int32_t* ok, bool* nothing) {
  *nothing = false;
  if (lanes == 0 || lanes > VDF_TAPE_MAX_LANES) return "lanes must be 1 .. VDF_TAPE_MAX_LANES";
  if (lanes * tp->n_inv > VDF_TAPE_MAX_INV) return "lanes * n_inv > VDF_TAPE_MAX_INV (all lanes' inv travel in the kernel arguments)";
  if (tp->n_inv && !inv) return "null inv";
  if (!j_base) return "null j_base";
  if (tp->n_slots + 2 * tp->n_adv + tp->n_inv + ti.chain_tmp > VDF_WALK_MAX_SLOTS)
    return "rebuild tape: n_slots + 2 * n_adv + n_inv + the chains' n_tmp > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)";
  if (rounds > VDF_FORWARD_TAPE_MAX_WORK / ti.products) return "rounds x products per round > VDF_FORWARD_TAPE_MAX_WORK in one call: cut the walk";
  if (expect && !ok) return "expect without ok";
  if (n == 0 || rounds == 0) { *nothing = true; return ""; }
  if (n > ((size_t)1 << 31)) return "more than 2^31 walks";
  if (!entries) return "null entries";
  if (trace && (group ? group : n) > 1 && (base > walk_stride || rounds > walk_stride - base))
    return "base + rounds > walk_stride: the walk would write into the run of the walk above it";
  return "";
}

}  // namespace vdfrebuild
