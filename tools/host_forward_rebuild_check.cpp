// Stand-alone driver of the host code of traces rebuilt by forward tapes (vdf_amd/csrc/tape_launch.h, host/rounds_host.cpp
// vdf_nova_forward_tape_rebuild_eval_lanes, host/custom_chain_host.cpp's ascending constructors) for the sanitizers: the restatement
// over a window laid out EXACTLY -- every array as long as the call may touch and no longer, so that an index one past its run is
// an error the sanitizer reports -- against one whole chain by vdf_nova_forward_tape_eval; the same with a table of three rows and
// a counter that crosses 2^64; every refusal with nothing written; the constructors' copies, refusals, direction and the clamp of
// launch_rounds.  No device is touched.  tools/host_forward_rebuild_sanitize.sh builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vdf_nova.h"

#define REQUIRE(cond)                                                                   \
  do {                                                                                  \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, vdf_nova_last_error()); return 1; } \
  } while (0)

struct Body { const vdf_fe* table; size_t rows; const uint64_t* e; };

// an entry is (a, b, c): a' = (a + b - k + j + tab[0])^5 by POW, b' = a^5 by a chain, c' = a' * tab[1] + c
static int forward_body(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* cur, vdf_num* out) {
  const Body* b = (const Body*)self;
  static const vdf_pow_step chain5[1] = {{0, 2, 0, VDF_POW_NONE}};
  vdf_num d = vdf_cs_add(cs, vdf_cs_sub(cs, vdf_cs_add(cs, cur[0], cur[1]), inv[0]), j);
  if (b->table) d = vdf_cs_add(cs, d, vdf_cs_tab(cs, b->table, b->rows, 2, 0));
  out[0] = vdf_cs_pow(cs, d, b->e);
  out[1] = vdf_cs_pow_chain(cs, cur[0], chain5, 1);
  out[2] = b->table ? vdf_cs_add(cs, vdf_cs_mul(cs, out[0], vdf_cs_tab(cs, b->table, b->rows, 2, 1)), cur[2]) : vdf_cs_add(cs, out[0], cur[2]);
  return 0;
}
static int walk_body(void*, vdf_cs* cs, vdf_num j, const vdf_num*, const vdf_num* next, vdf_num* out) {
  out[0] = vdf_cs_add(cs, next[0], j);
  out[1] = next[1];
  out[2] = next[2];
  return 0;
}

static bool same(const vdf_fe* a, const vdf_fe* b, size_t n) { return memcmp(a, b, n * sizeof(vdf_fe)) == 0; }

// One window of `steps` steps of `lanes` lanes at t = group * every, in slices of 2 + 2 + 1, from arrays of exactly the sizes the
// call may touch; compared with whole chains.  0: all as expected.
static int window(int F, const vdf_round_tape* tape, size_t lanes, size_t group, const uint64_t* j_base, int heads) {
  const size_t na = 3, every = 5, steps = 2, t = group * every, n = steps * lanes * group;
  std::vector<vdf_fe> inv(lanes);
  for (size_t l = 0; l < lanes; ++l) inv[l] = vdf_fe{{3 + 10 * l, 0, 0, 0}};
  // the oracle: one chain per lane from entry 0, trace on
  std::vector<std::vector<vdf_fe>> chains(lanes);
  for (size_t l = 0; l < lanes; ++l) {
    chains[l].assign((steps * t + 1) * na, vdf_fe{{0, 0, 0, 0}});
    for (size_t c = 0; c < na; ++c) chains[l][c] = vdf_fe{{7 + l + c, c, 0, 0}};
    std::vector<vdf_fe> e(chains[l].begin(), chains[l].begin() + na);
    REQUIRE(vdf_nova_forward_tape_eval(F, tape, &inv[l], e.data(), 1, steps * t, nullptr, 0, 0, chains[l].data(), 0, 0, j_base[l], 0) == VDF_OK);
  }
  std::vector<vdf_fe> entries(n * na), expect(n * na), trace(steps * lanes * (t + 1) * na, vdf_fe{{~0ull, ~0ull, ~0ull, ~0ull}});
  std::vector<int32_t> ok(n, -7);
  for (size_t w = 0; w < n; ++w) {
    const size_t G = w / group, g = G / lanes, l = G % lanes, k = g * t + (w % group) * every;
    memcpy(&entries[w * na], &chains[l][k * na], na * sizeof(vdf_fe));
    memcpy(&expect[w * na], &chains[l][(k + every) * na], na * sizeof(vdf_fe));
  }
  const uint64_t slices[3] = {2, 2, 1};
  uint64_t base = 0;
  for (int s = 0; s < 3; ++s) {
    REQUIRE(vdf_nova_forward_tape_rebuild_eval_lanes(F, tape, lanes, inv.data(), entries.data(), n, slices[s], trace.data(), every, base, group, t + 1,
                                                     j_base, t, heads, s == 2 ? expect.data() : nullptr, s == 2 ? ok.data() : nullptr) == VDF_OK);
    base += slices[s];
  }
  REQUIRE(same(entries.data(), expect.data(), n * na));
  for (size_t w = 0; w < n; ++w) REQUIRE(ok[w] == 1);
  for (size_t G = 0; G < steps * lanes; ++G) {
    const size_t g = G / lanes, l = G % lanes, lo = heads ? 0 : 1;
    REQUIRE(same(&trace[(G * (t + 1) + lo) * na], &chains[l][(g * t + lo) * na], (t + 1 - lo) * na));
    if (!heads) REQUIRE(trace[G * (t + 1) * na].l[0] == ~0ull);
  }
  return 0;
}

int main() {
  const int F = VDF_FIELD_FQ;
  const uint64_t five[4] = {5, 0, 0, 0};
  std::vector<vdf_fe> small(3 * 2);
  for (size_t k = 0; k < small.size(); ++k) small[k] = vdf_fe{{100 + k, 0, 0, 0}};
  Body plain = {nullptr, 0, five}, tabbed = {small.data(), 3, five};
  static vdf_tape_op ops[3][VDF_TAPE_MAX_OPS];
  static vdf_fe consts[3][VDF_TAPE_MAX_CONSTS];
  vdf_round_tape fwd, ftab, walk;
  const vdf_walk_body fb = {1, 3, forward_body, &plain}, tb = {1, 3, forward_body, &tabbed}, wb = {0, 3, walk_body, nullptr};
  REQUIRE(vdf_nova_forward_body_record(F, &fb, ops[0], consts[0], &fwd) == VDF_OK);
  REQUIRE(vdf_nova_forward_body_record(F, &tb, ops[1], consts[1], &ftab) == VDF_OK && ftab.tab_rows == 3);
  REQUIRE(vdf_nova_walk_body_record(F, &wb, ops[2], consts[2], &walk) == VDF_OK);

  // ---- windows laid out exactly: one lane and three, groups of 2 and 4, with and without heads, a counter that crosses 2^64 ----
  const uint64_t jb[3] = {~0ull - 2, 997, 12};                      // lane 0: 2^64 - 3
  for (const vdf_round_tape* tp : {&fwd, &ftab})
    for (size_t lanes : {(size_t)1, (size_t)3})
      for (size_t group : {(size_t)2, (size_t)4})
        for (int heads = 0; heads < 2; ++heads)
          if (window(F, tp, lanes, group, jb, heads)) return 1;

  // ---- every refusal: nothing is written ----
  {
    const vdf_fe guard = {{~0ull, ~0ull, ~0ull, ~0ull}};
    std::vector<vdf_fe> e(4 * 3, guard), tr(64, guard), inv(16, small[0]);
    std::vector<int32_t> ok(4, -7);
    const uint64_t one = 1;
    auto untouched = [&]() {
      for (const vdf_fe& v : e) if (v.l[0] != ~0ull) return false;
      for (const vdf_fe& v : tr) if (v.l[0] != ~0ull) return false;
      return ok[0] == -7;
    };
    auto call = [&](const vdf_round_tape* tp, size_t lanes, const uint64_t* j, size_t n, uint64_t rounds, vdf_fe* trace, size_t stride, uint64_t base,
                    size_t group, const vdf_fe* expect, int32_t* okp, const char* text) {
      const int rc = vdf_nova_forward_tape_rebuild_eval_lanes(F, tp, lanes, inv.data(), e.data(), n, rounds, trace, stride, base, group, 16, j, 0, 1, expect, okp);
      return rc == VDF_ERR_BAD_ARG && strstr(vdf_nova_last_error(), text) != nullptr && untouched();
    };
    REQUIRE(call(&walk, 1, &one, 1, 1, nullptr, 0, 0, 0, nullptr, nullptr, "b = 0 only"));
    REQUIRE(call(&fwd, 0, &one, 1, 1, nullptr, 0, 0, 0, nullptr, nullptr, "lanes must be"));
    REQUIRE(call(&fwd, VDF_TAPE_MAX_LANES + 1, &one, 1, 1, nullptr, 0, 0, 0, nullptr, nullptr, "lanes must be"));
    REQUIRE(call(&fwd, 1, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, nullptr, "null j_base"));
    REQUIRE(call(&fwd, 1, &one, 1, 1, nullptr, 0, 0, 0, e.data(), nullptr, "expect without ok"));
    REQUIRE(call(&fwd, 1, &one, 4, 3, tr.data(), 5, 3, 2, nullptr, nullptr, "base + rounds > walk_stride"));
    REQUIRE(call(&fwd, 1, &one, 0, VDF_FORWARD_TAPE_MAX_WORK, nullptr, 0, 0, 0, nullptr, nullptr, "VDF_FORWARD_TAPE_MAX_WORK"));
    REQUIRE(vdf_nova_forward_tape_rebuild_eval_lanes(F, &fwd, 1, nullptr, e.data(), 1, 1, nullptr, 0, 0, 0, 0, &one, 0, 0, nullptr, nullptr) == VDF_ERR_BAD_ARG);
    REQUIRE(strstr(vdf_nova_last_error(), "null inv") != nullptr && untouched());
    REQUIRE(vdf_nova_forward_tape_rebuild_eval_lanes(F, nullptr, 1, nullptr, e.data(), 1, 1, nullptr, 0, 0, 0, 0, &one, 0, 0, nullptr, nullptr) == VDF_ERR_BAD_ARG);
    // n = 0 and rounds = 0 do nothing, also over null arrays
    REQUIRE(vdf_nova_forward_tape_rebuild_eval_lanes(F, &fwd, 1, inv.data(), nullptr, 0, 5, nullptr, 0, 0, 0, 0, &one, 0, 1, nullptr, nullptr) == VDF_OK);
    REQUIRE(vdf_nova_forward_tape_rebuild_eval_lanes(F, &fwd, 1, inv.data(), nullptr, 5, 0, nullptr, 0, 0, 0, 0, &one, 0, 1, nullptr, nullptr) == VDF_OK);
  }

  // ---- the constructors: copies, refusals, direction, the clamp ----
  {
    std::vector<vdf_fe> cps(3 * 7 * 3, small[0]), inv(3, small[1]);
    vdf_custom_chain* chain = nullptr;
    uint64_t bytes = 0, lr = 0;
    REQUIRE(vdf_nova_custom_chain_from_checkpoints_forward(F, &ftab, inv.data(), 6, 3, 3, cps.data(), 3, &chain) == VDF_OK);
    REQUIRE(vdf_nova_custom_chain_direction(chain) == VDF_CHAIN_ASCENDING && vdf_nova_custom_chain_len(chain) == 3);
    REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK && bytes >= (6 + 1 + 7 * 3) * 32);
    REQUIRE(vdf_nova_custom_chain_launch_rounds(chain, 0, &lr) == VDF_OK && lr == 1024);
    REQUIRE(vdf_nova_custom_chain_launch_rounds(chain, 1u << 20, &lr) == VDF_OK && lr == 1024);
    REQUIRE(vdf_nova_custom_chain_set_launch_rounds(chain, 3) == VDF_OK && vdf_nova_custom_chain_launch_rounds(chain, 0, &lr) == VDF_OK && lr == 3);
    vdf_nova_custom_chain_free(chain);
    const uint64_t jb3[3] = {0, 3, 6};
    REQUIRE(vdf_nova_custom_chain_lanes_from_checkpoints_forward(F, &ftab, inv.data(), 6, 3, 3, 3, cps.data(), 7, jb3, &chain) == VDF_OK);
    REQUIRE(vdf_nova_custom_chain_direction(chain) == VDF_CHAIN_ASCENDING);
    vdf_nova_custom_chain_free(chain);
    REQUIRE(vdf_nova_custom_chain_from_checkpoints_forward(F, &walk, nullptr, 6, 3, 3, cps.data(), 0, &chain) == VDF_ERR_BAD_ARG && !chain);
    REQUIRE(vdf_nova_custom_chain_from_checkpoints_forward(F, &ftab, inv.data(), 8, 4, 1, cps.data(), 0, &chain) == VDF_ERR_BAD_ARG && !chain);
    REQUIRE(strstr(vdf_nova_last_error(), "must divide t") != nullptr);
    REQUIRE(vdf_nova_custom_chain_from_checkpoints_forward(F, &ftab, inv.data(), 6, 3, 3, cps.data(), 4, &chain) == VDF_ERR_BAD_ARG && !chain);
    REQUIRE(strstr(vdf_nova_last_error(), "must divide every j_base") != nullptr);
    REQUIRE(vdf_nova_custom_chain_from_checkpoints(F, &fwd, inv.data(), 6, 3, 3, cps.data(), 0, &chain) == VDF_ERR_BAD_ARG && !chain);      // a POW in a walk tape
    REQUIRE(vdf_nova_custom_chain_from_checkpoints(F, &walk, nullptr, 6, 3, 3, cps.data(), 0, &chain) == VDF_OK);
    REQUIRE(vdf_nova_custom_chain_direction(chain) == VDF_CHAIN_DESCENDING && vdf_nova_custom_chain_direction(nullptr) == -1);
    REQUIRE(vdf_nova_custom_chain_launch_rounds(chain, 5000, &lr) == VDF_OK && lr == 5000);
    vdf_nova_custom_chain_free(chain);
  }
  printf("host forward rebuild: ok\n");
  return 0;
}
