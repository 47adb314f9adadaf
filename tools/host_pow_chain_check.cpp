// Stand-alone driver of the host code of caller-supplied addition chains (vdf_amd/csrc/pow_chain.h, host/rounds_host.cpp) for the
// sanitizers: the chain validation with its refusals, the sliding-window generator against the exponent it was asked for, the
// library's own MinRoot chains, the recorder (vdf_cs_pow_chain in a forward body, and where it is refused) and the host evaluator
// over the MinRoot tape by POW, by the reference's chain and by a window chain.  No device is touched.
// tools/host_pow_chain_sanitize.sh builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vdf_nova.h"

#define REQUIRE(cond)                                                                   \
  do {                                                                                  \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, vdf_nova_last_error()); return 1; } \
  } while (0)

struct Root { const vdf_pow_step* steps; size_t n; const uint64_t* e; };
// entry j = (x, y) -> entry j + 1 = ((x + y)^(1/5), x + j): the root by a chain, or by square-and-multiply (steps == nullptr)
static int forward_body(void* self, vdf_cs* cs, vdf_num j, const vdf_num*, const vdf_num* cur, vdf_num* out) {
  const Root* r = (const Root*)self;
  const vdf_num s = vdf_cs_add(cs, cur[0], cur[1]);
  out[0] = r->steps ? vdf_cs_pow_chain(cs, s, r->steps, r->n) : vdf_cs_pow(cs, s, r->e);
  out[1] = vdf_cs_add(cs, cur[0], j);
  return 0;
}
static int descending_body(void* self, vdf_cs* cs, vdf_num, const vdf_num*, const vdf_num* next, vdf_num* out) {
  const Root* r = (const Root*)self;
  out[0] = vdf_cs_pow_chain(cs, next[0], r->steps, r->n);
  out[1] = next[1];
  return 0;
}

int main() {
  const vdf_pow_step ok[] = {{0, 1, VDF_POW_NONE, 1}, {VDF_POW_ACC, 0, 1, VDF_POW_NONE}};      // x^4 through T[1]
  uint64_t e[4], products = 0;
  uint32_t n_tmp = 0;
  size_t n = 0;
  // ---- validation and its refusals, a valid call after each ----
  std::vector<std::vector<vdf_pow_step>> bad = {
      {{VDF_POW_ACC, 1, VDF_POW_NONE, VDF_POW_NONE}},
      {{0, 1, VDF_POW_NONE, 1}, {2, 0, VDF_POW_NONE, VDF_POW_NONE}},
      {{0, 1, 1, VDF_POW_NONE}},
      {{0, 1, VDF_POW_NONE, VDF_POW_CHAIN_MAX_TMP}},
      {{0, 255, VDF_POW_NONE, 1}, {VDF_POW_ACC, 1, VDF_POW_NONE, VDF_POW_NONE}},
      {{0, 255, VDF_POW_NONE, 1}, {VDF_POW_ACC, 0, 1, VDF_POW_NONE}},
      std::vector<vdf_pow_step>(VDF_POW_CHAIN_MAX_STEPS + 1, vdf_pow_step{0, 0, VDF_POW_NONE, VDF_POW_NONE}),
  };
  for (const auto& c : bad) {
    REQUIRE(vdf_nova_pow_chain_exponent(c.data(), c.size(), e, &n_tmp, &products) == VDF_ERR_BAD_ARG);
    REQUIRE(vdf_nova_pow_chain_exponent(ok, 2, e, &n_tmp, &products) == VDF_OK && e[0] == 4 && n_tmp == 2 && products == 2);
  }
  REQUIRE(vdf_nova_pow_chain_exponent(ok, 0, e, nullptr, nullptr) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_pow_chain_exponent(nullptr, 2, e, nullptr, nullptr) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_pow_chain_exponent(ok, 2, nullptr, nullptr, nullptr) == VDF_OK);
  std::vector<vdf_pow_step> longest(VDF_POW_CHAIN_MAX_STEPS, vdf_pow_step{0, 0, VDF_POW_NONE, VDF_POW_NONE});
  REQUIRE(vdf_nova_pow_chain_exponent(longest.data(), longest.size(), e, &n_tmp, &products) == VDF_OK && e[0] == 1 && products == 1);

  // ---- the generator: the exponent comes back, for every window; its refusals ----
  vdf_pow_step steps[VDF_POW_CHAIN_MAX_STEPS];
  const uint64_t exps[][4] = {{1, 0, 0, 0}, {2, 0, 0, 0}, {3, 0, 0, 0}, {0, 0, 0, 1ull << 63}, {~0ull, ~0ull, ~0ull, ~0ull >> 1},
                              {~0ull, ~0ull, ~0ull, ~0ull}, {0x123456789abcdef0ull, 0, 0xfedcba9876543210ull, 0x0fffffff00000001ull}};
  for (const auto& x : exps)
    for (unsigned w = 2; w <= 4; ++w) {
      const int rc = vdf_nova_pow_chain_window(x, w, steps, VDF_POW_CHAIN_MAX_STEPS, &n);
      if (rc == VDF_ERR_BAD_LENGTH) continue;                   // a dense exponent at a small window
      REQUIRE(rc == VDF_OK);
      REQUIRE(vdf_nova_pow_chain_exponent(steps, n, e, &n_tmp, &products) == VDF_OK && memcmp(e, x, 32) == 0 && n_tmp == (1u << (w - 1)) + 1);
      REQUIRE(vdf_nova_pow_chain_window(x, w, steps, n - 1, &n) == VDF_ERR_BAD_LENGTH);
    }
  const uint64_t zero[4] = {0, 0, 0, 0};
  REQUIRE(vdf_nova_pow_chain_window(zero, 4, steps, VDF_POW_CHAIN_MAX_STEPS, &n) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_pow_chain_window(exps[2], 1, steps, VDF_POW_CHAIN_MAX_STEPS, &n) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_pow_chain_window(exps[2], 5, steps, VDF_POW_CHAIN_MAX_STEPS, &n) == VDF_ERR_BAD_ARG);

  // ---- the library's chains, the recorder and the evaluator, both fields ----
  for (int F : {VDF_FIELD_FQ, VDF_FIELD_FP}) {
    vdf_pow_step own[32], win[VDF_POW_CHAIN_MAX_STEPS];
    size_t n_own = 0, n_win = 0;
    REQUIRE(vdf_minroot_pow_chain(F, own, 31, &n_own) == VDF_ERR_BAD_LENGTH);
    REQUIRE(vdf_minroot_pow_chain(F, own, 32, &n_own) == VDF_OK && n_own == 32);
    uint64_t root[4];
    REQUIRE(vdf_nova_pow_chain_exponent(own, n_own, root, &n_tmp, &products) == VDF_OK && n_tmp == 9);
    REQUIRE(products == (F == VDF_FIELD_FQ ? 283u : 282u));
    REQUIRE(vdf_nova_pow_chain_window(root, 4, win, VDF_POW_CHAIN_MAX_STEPS, &n_win) == VDF_OK);
    REQUIRE(vdf_nova_pow_chain_exponent(win, n_win, e, nullptr, &products) == VDF_OK && memcmp(e, root, 32) == 0 && products == 316);

    static vdf_tape_op ops[3][VDF_TAPE_MAX_OPS];
    static vdf_fe consts[3][VDF_TAPE_MAX_CONSTS];
    vdf_round_tape tape[3];
    Root how[3] = {{nullptr, 0, root}, {own, n_own, root}, {win, n_win, root}};
    for (int k = 0; k < 3; ++k) {
      const vdf_walk_body b = {0, 2, forward_body, &how[k]};
      REQUIRE(vdf_nova_forward_body_record(F, &b, ops[k], consts[k], &tape[k]) == VDF_OK);
    }
    REQUIRE(tape[1].n_consts == 5 && tape[1].n_ops == tape[0].n_ops);
    // an invalid chain, and a chain in a descending body, set the failure flag
    Root broken = {bad[1].data(), bad[1].size(), root};
    const vdf_walk_body bb = {0, 2, forward_body, &broken}, db = {0, 2, descending_body, &how[1]};
    static vdf_tape_op o2[VDF_TAPE_MAX_OPS];
    static vdf_fe c2[VDF_TAPE_MAX_CONSTS];
    vdf_round_tape t2;
    REQUIRE(vdf_nova_forward_body_record(F, &bb, o2, c2, &t2) == VDF_ERR_BAD_ARG);
    REQUIRE(vdf_nova_walk_body_record(F, &db, o2, c2, &t2) == VDF_ERR_BAD_ARG);

    const size_t nw = 3, rounds = 7, every = 1, stride = rounds + 2;
    std::vector<vdf_fe> out[3][3];
    for (int k = 0; k < 3; ++k) {
      std::vector<vdf_fe> entries(2 * nw), cps(2 * nw * stride), trace(2 * nw * stride);
      for (size_t w = 0; w < nw; ++w) {
        REQUIRE(vdf_minroot_element(F, w ? 1000 + w : 5, &entries[2 * w]) == VDF_OK);
        REQUIRE(vdf_minroot_element(F, 77 * w, &entries[2 * w + 1]) == VDF_OK);
      }
      memset(cps.data(), 0xff, cps.size() * sizeof(vdf_fe));
      memset(trace.data(), 0xff, trace.size() * sizeof(vdf_fe));
      REQUIRE(vdf_nova_forward_tape_eval(F, &tape[k], nullptr, entries.data(), nw, rounds, cps.data(), every, stride, trace.data(), stride, 0, 9,
                                         100) == VDF_OK);
      out[k][0] = entries; out[k][1] = cps; out[k][2] = trace;
    }
    for (int k = 1; k < 3; ++k)
      for (int q = 0; q < 3; ++q) REQUIRE(memcmp(out[k][q].data(), out[0][q].data(), out[0][q].size() * sizeof(vdf_fe)) == 0);
    // the packed chain tampered with: padding, a step, the count of constants -- refused, and the tape as it was runs again
    std::vector<vdf_fe> entries(2 * nw);
    memcpy(entries.data(), out[0][0].data(), entries.size() * sizeof(vdf_fe));
    uint8_t* raw = (uint8_t*)consts[1];
    const struct { size_t at; uint8_t v; } tamper[] = {{4, VDF_POW_ACC}, {1, 13}, {0, 96}, {2, 1}, {4 + 128, 1}, {5 * 32 - 1, 1}};
    for (const auto& t : tamper) {
      const uint8_t was = raw[t.at];
      raw[t.at] = t.v;
      REQUIRE(vdf_nova_forward_tape_eval(F, &tape[1], nullptr, entries.data(), nw, 1, nullptr, 0, 0, nullptr, 0, 0, 0, 0) == VDF_ERR_BAD_ARG);
      raw[t.at] = was;
    }
    tape[1].n_consts = 4;
    REQUIRE(vdf_nova_forward_tape_eval(F, &tape[1], nullptr, entries.data(), nw, 1, nullptr, 0, 0, nullptr, 0, 0, 0, 0) == VDF_ERR_BAD_ARG);
    tape[1].n_consts = 5;
    REQUIRE(memcmp(entries.data(), out[0][0].data(), entries.size() * sizeof(vdf_fe)) == 0);
    REQUIRE(vdf_nova_forward_tape_eval(F, &tape[1], nullptr, entries.data(), nw, 1, nullptr, 0, 0, nullptr, 0, 0, 0, 0) == VDF_OK);
  }
  printf("host pow-chain check: ok\n");
  return 0;
}
