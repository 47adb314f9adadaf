// Stand-alone driver of the host code of custom chains that grow (host/custom_chain_host.cpp: vdf_nova_custom_chain_begin,
// _push_checkpoints, _push_advice) and of the evaluator behind vdf_nova_eval_and_prove_custom (host/custom_stream.hpp), for the
// sanitizers: chains grown by both hand-overs for one lane and three, every refusal of the push calls with nothing appended, release
// and free; the evaluator run to completion against whole chains by vdf_nova_forward_tape_eval, and with a consumer that stops after
// the first step.  No device is touched.  tools/host_custom_stream_sanitize.sh builds and runs it (argument "evaluator": that part
// alone, what the thread sanitizer's build runs).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vdf_nova.h"
#include "../vdf_amd/csrc/host/custom_stream.hpp"

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

static const int F = VDF_FIELD_FQ;
static const size_t NA = 3;
static bool same(const vdf_fe* a, const vdf_fe* b, size_t n) { return memcmp(a, b, n * sizeof(vdf_fe)) == 0; }
static bool says(const char* text) { return strstr(vdf_nova_last_error(), text) != nullptr; }

// `lanes` whole chains of steps * t rounds by vdf_nova_forward_tape_eval: chains[l] = steps * t + 1 entries
static int whole_chains(const vdf_round_tape* tape, size_t lanes, uint64_t t, size_t steps, const vdf_fe* inv, const uint64_t* j_base,
                        std::vector<std::vector<vdf_fe>>* chains) {
  chains->assign(lanes, std::vector<vdf_fe>());
  for (size_t l = 0; l < lanes; ++l) {
    std::vector<vdf_fe>& c = (*chains)[l];
    c.assign((steps * t + 1) * NA, vdf_fe{{0, 0, 0, 0}});
    for (size_t k = 0; k < NA; ++k) c[k] = vdf_fe{{7 + l + k, k, 0, 0}};
    std::vector<vdf_fe> e(c.begin(), c.begin() + NA);
    REQUIRE(vdf_nova_forward_tape_eval(F, tape, inv + l, e.data(), 1, steps * t, nullptr, 0, 0, c.data(), 0, 0, j_base[l], 0) == VDF_OK);
  }
  return 0;
}

// one step of every lane as a push takes it: lanes runs of `entries` entries, `stride` rounds apart, lane l's at l * lane_stride
static std::vector<vdf_fe> step_of(const std::vector<std::vector<vdf_fe>>& chains, size_t k, uint64_t t, size_t entries, size_t stride, size_t lane_stride) {
  std::vector<vdf_fe> out(chains.size() * lane_stride * NA, vdf_fe{{~0ull, 0, 0, 0}});
  for (size_t l = 0; l < chains.size(); ++l)
    for (size_t e = 0; e < entries; ++e) memcpy(&out[(l * lane_stride + e) * NA], &chains[l][(k * t + e * stride) * NA], NA * sizeof(vdf_fe));
  return out;
}

// ---- chains that grow: both hand-overs, lanes 1 and 3, every refusal, release and free ----
static int growing(const vdf_round_tape* fwd, const vdf_round_tape* ftab, const vdf_round_tape* walk) {
  const uint64_t t = 6, every = 3;
  const size_t steps = 3;
  const uint64_t jb[3] = {0, 3, 12};
  for (size_t lanes : {(size_t)1, (size_t)3}) {
    std::vector<vdf_fe> inv(lanes);
    for (size_t l = 0; l < lanes; ++l) inv[l] = vdf_fe{{3 + 10 * l, 0, 0, 0}};
    std::vector<std::vector<vdf_fe>> chains;
    if (whole_chains(ftab, lanes, t, steps, inv.data(), jb, &chains)) return 1;
    std::vector<vdf_fe> initial(lanes * NA);
    for (size_t l = 0; l < lanes; ++l) memcpy(&initial[l * NA], chains[l].data(), NA * sizeof(vdf_fe));
    const size_t per = t / every;
    for (int advice = 0; advice < 2; ++advice)
      for (int direction : {VDF_CHAIN_ASCENDING, VDF_CHAIN_DESCENDING}) {
        vdf_custom_chain* chain = nullptr;
        const vdf_round_tape* tape = direction == VDF_CHAIN_ASCENDING ? ftab : walk;
        REQUIRE(vdf_nova_custom_chain_begin(F, tape, direction, inv.data(), t, lanes, initial.data(), jb, &chain) == VDF_OK && chain);
        REQUIRE(vdf_nova_custom_chain_len(chain) == 0 && vdf_nova_custom_chain_direction(chain) == direction);
        uint64_t bytes0 = 0, bytes = 0;
        REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes0) == VDF_OK && bytes0 >= lanes * NA * 32);
        const size_t entries = advice ? t + 1 : per + 1, stride = advice ? 1 : every, ls = entries + 2;      // lanes apart by more than they need
        for (size_t k = 0; k < steps; ++k) {
          // a step that does not start on the chain's end: the wrong lane is named and nothing is appended
          std::vector<vdf_fe> bad = step_of(chains, k, t, entries, stride, ls);
          bad[((lanes - 1) * ls) * NA + 1].l[0] ^= 1;
          const int rc_bad = advice ? vdf_nova_custom_chain_push_advice(chain, bad.data(), ls) : vdf_nova_custom_chain_push_checkpoints(chain, every, bad.data(), ls);
          REQUIRE(rc_bad == VDF_ERR_BAD_ARG && says(("lane " + std::to_string(lanes - 1) + ": the step does not start on the chain's end").c_str()));
          REQUIRE(vdf_nova_custom_chain_len(chain) == k);
          // the step itself, from an array laid out exactly: an index past a lane's run is the sanitizer's to report
          const std::vector<vdf_fe> good = step_of(chains, k, t, entries, stride, lanes == 1 ? entries : ls);
          std::vector<vdf_fe> exact(good.begin(), good.begin() + ((lanes - 1) * (lanes == 1 ? entries : ls) + entries) * NA);
          const size_t stride_arg = lanes == 1 ? 0 : ls;                                                     // (not read for one lane)
          REQUIRE((advice ? vdf_nova_custom_chain_push_advice(chain, exact.data(), stride_arg)
                          : vdf_nova_custom_chain_push_checkpoints(chain, every, exact.data(), stride_arg)) == VDF_OK);
          REQUIRE(vdf_nova_custom_chain_len(chain) == k + 1);
          // one hand-over per chain, one `every` per chain
          if (advice) REQUIRE(vdf_nova_custom_chain_push_checkpoints(chain, every, exact.data(), stride_arg) == VDF_ERR_BAD_ARG && says("one hand-over per chain"));
          else {
            REQUIRE(vdf_nova_custom_chain_push_advice(chain, exact.data(), stride_arg) == VDF_ERR_BAD_ARG && says("one hand-over per chain"));
            REQUIRE(vdf_nova_custom_chain_push_checkpoints(chain, 2, exact.data(), stride_arg) == VDF_ERR_BAD_ARG && says("the chain's first push said 3"));
            REQUIRE(vdf_nova_custom_chain_push_checkpoints(chain, 4, exact.data(), stride_arg) == VDF_ERR_BAD_ARG && says("must be positive and divide t"));
          }
          REQUIRE(vdf_nova_custom_chain_len(chain) == k + 1);
          REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK);
          REQUIRE(bytes == bytes0 + (k + 1) * lanes * (advice ? t + 1 : per) * NA * 32);
        }
        if (lanes > 1) {
          const std::vector<vdf_fe> next = step_of(chains, 0, t, entries, stride, ls);
          REQUIRE((advice ? vdf_nova_custom_chain_push_advice(chain, next.data(), entries - 1)
                          : vdf_nova_custom_chain_push_checkpoints(chain, every, next.data(), entries - 1)) == VDF_ERR_BAD_ARG && says("lane_stride must be at least"));
        }
        // release: the host copies of traces go, checkpoints stay; out of range is refused
        REQUIRE(vdf_nova_custom_chain_release(chain, 0, 2) == VDF_OK);
        REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK);
        REQUIRE(bytes == bytes0 + (advice ? 1 : steps) * lanes * (advice ? t + 1 : per) * NA * 32);
        REQUIRE(vdf_nova_custom_chain_release(chain, 2, 2) == VDF_ERR_BAD_LENGTH);
        REQUIRE(vdf_nova_custom_chain_release(chain, 2, 1) == VDF_OK);
        REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK && bytes == bytes0 + (advice ? 0 : steps * lanes * per * NA * 32));
        size_t resident = 7;
        uint64_t dev_bytes = 7;
        REQUIRE(vdf_nova_custom_chain_memory(chain, &resident, &dev_bytes) == VDF_OK && resident == 0 && dev_bytes == 0);
        vdf_nova_custom_chain_free(chain);
      }
  }
  // ---- begin's refusals, and the push calls on a chain made whole ----
  {
    const vdf_fe one = {{1, 0, 0, 0}};
    std::vector<vdf_fe> initial(3 * NA, one), inv(3, one), cps(3 * 7 * NA, one);
    const uint64_t jb3[3] = {0, 3, 6}, odd[3] = {0, 4, 6};
    vdf_custom_chain* chain = (vdf_custom_chain*)&one;
    auto refused = [&](int rc, const char* text) { return rc == VDF_ERR_BAD_ARG && chain == nullptr && says(text); };
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, 2, inv.data(), t, 3, initial.data(), jb3, &chain), "direction must be"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(7, ftab, VDF_CHAIN_ASCENDING, inv.data(), t, 3, initial.data(), jb3, &chain), "unknown field"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, nullptr, VDF_CHAIN_ASCENDING, inv.data(), t, 3, initial.data(), jb3, &chain), "null argument"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, inv.data(), t, 3, nullptr, jb3, &chain), "null argument"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, inv.data(), t, 3, initial.data(), nullptr, &chain), "null argument"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, inv.data(), 0, 3, initial.data(), jb3, &chain), "t out of range"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, inv.data(), t, 0, initial.data(), jb3, &chain), "lanes must be"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, inv.data(), t, VDF_TAPE_MAX_LANES + 1, initial.data(), jb3, &chain), "lanes must be"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, nullptr, t, 3, initial.data(), jb3, &chain), "null inv"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, walk, VDF_CHAIN_ASCENDING, nullptr, t, 1, initial.data(), jb3, &chain), ""));          // a walk tape is no forward tape
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, fwd, VDF_CHAIN_DESCENDING, inv.data(), t, 1, initial.data(), jb3, &chain), ""));       // a POW in a walk tape
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, inv.data(), 8, 3, initial.data(), jb3, &chain), "tab_rows must divide t"));
    REQUIRE(refused(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, inv.data(), t, 3, initial.data(), odd, &chain), "tab_rows must divide every j_base"));
    REQUIRE(vdf_nova_custom_chain_begin(F, ftab, VDF_CHAIN_ASCENDING, inv.data(), t, 3, initial.data(), jb3, nullptr) == VDF_ERR_BAD_ARG);
    REQUIRE(vdf_nova_custom_chain_push_advice(nullptr, cps.data(), 7) == VDF_ERR_BAD_ARG);
    REQUIRE(vdf_nova_custom_chain_lanes_from_checkpoints_forward(F, ftab, inv.data(), t, 3, 3, 3, cps.data(), 7, jb3, &chain) == VDF_OK);
    REQUIRE(vdf_nova_custom_chain_push_checkpoints(chain, 3, cps.data(), 7) == VDF_ERR_BAD_ARG && says("only a chain of vdf_nova_custom_chain_begin grows"));
    REQUIRE(vdf_nova_custom_chain_push_advice(chain, cps.data(), 7) == VDF_ERR_BAD_ARG && says("only a chain of vdf_nova_custom_chain_begin grows"));
    REQUIRE(vdf_nova_custom_chain_len(chain) == 3);
    vdf_nova_custom_chain_free(chain);
  }
  return 0;
}

// ---- the evaluator: to completion against whole chains, and with a consumer that stops after the first step ----
static int evaluator(const vdf_round_tape* ftab) {
  using vdfnova::ChainEvaluator;
  const uint64_t t = 6;
  const size_t steps = 7;                                // more than the queue holds: the lanes wait for the taker
  const uint64_t jb[3] = {~0ull - 3, 3, 12};             // lane 0's counter crosses 2^64 (tab_rows = 3 divides 2^64 - 4)
  for (size_t lanes : {(size_t)1, (size_t)3})
    for (uint64_t every : {(uint64_t)0, (uint64_t)3}) {
      std::vector<vdf_fe> inv(lanes);
      for (size_t l = 0; l < lanes; ++l) inv[l] = vdf_fe{{3 + 10 * l, 0, 0, 0}};
      std::vector<std::vector<vdf_fe>> chains;
      if (whole_chains(ftab, lanes, t, steps, inv.data(), jb, &chains)) return 1;
      std::vector<vdf_fe> initial(lanes * NA);
      for (size_t l = 0; l < lanes; ++l) memcpy(&initial[l * NA], chains[l].data(), NA * sizeof(vdf_fe));
      const ChainEvaluator::Spec spec = {F, ftab, inv.data(), t, every, lanes, jb, steps, 4};
      {
        ChainEvaluator ev(spec, initial.data());
        const size_t entries = ev.entries(), stride = every ? every : 1;
        REQUIRE(entries == (every ? t / every + 1 : t + 1));
        ev.start();
        std::vector<ChainEvaluator::Step> got;
        std::string why;
        size_t backlog = 0;
        while (got.size() < steps) {
          const size_t before = got.size();
          REQUIRE(ev.take(&got, true, &why) == VDF_OK);
          REQUIRE(got.size() > before && got.size() - before <= 4);
          backlog = std::max(backlog, got.size() - before);
        }
        REQUIRE(ev.take(&got, true, &why) == VDF_OK && got.size() == steps);      // everything taken: returns at once
        for (size_t k = 0; k < steps; ++k) {
          REQUIRE(got[k].size() == lanes * entries * NA);
          REQUIRE(same(got[k].data(), step_of(chains, k, t, entries, stride, entries).data(), lanes * entries * NA));
        }
        double ms = 0, end = 0;
        ev.eval_times(&ms, &end);
        REQUIRE(ms > 0 && end > 0 && backlog >= 1);
      }
      {                                                  // a consumer that stops after the first step: the lanes end, nothing leaks
        ChainEvaluator ev(spec, initial.data());
        ev.start();
        std::vector<ChainEvaluator::Step> got;
        std::string why;
        REQUIRE(ev.take(&got, true, &why) == VDF_OK && !got.empty());
        REQUIRE(same(got[0].data(), step_of(chains, 0, t, ev.entries(), every ? every : 1, ev.entries()).data(), lanes * ev.entries() * NA));
        ev.stop();
        ev.join();
        REQUIRE(ev.take(&got, true, &why) == VDF_OK);    // stopped: never blocks
      }
      { ChainEvaluator never_started(spec, initial.data()); }
    }
  // a lane that fails (the tape reads inv, none is given) is the taker's error, with the lane named
  {
    const vdf_fe initial[NA] = {{{1, 0, 0, 0}}, {{2, 0, 0, 0}}, {{3, 0, 0, 0}}};
    const ChainEvaluator::Spec spec = {F, ftab, nullptr, t, 0, 1, jb, 2, 4};
    ChainEvaluator ev(spec, initial);
    ev.start();
    std::vector<ChainEvaluator::Step> got;
    std::string why;
    REQUIRE(ev.take(&got, true, &why) == VDF_ERR_BAD_ARG && got.empty() && why.find("lane 0: ") == 0);
  }
  return 0;
}

int main(int argc, char** argv) {
  const bool only_evaluator = argc > 1 && strcmp(argv[1], "evaluator") == 0;
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
  if (!only_evaluator && growing(&fwd, &ftab, &walk)) return 1;
  if (evaluator(&ftab)) return 1;
  printf("host custom stream%s: ok\n", only_evaluator ? " (evaluator)" : "");
  return 0;
}
