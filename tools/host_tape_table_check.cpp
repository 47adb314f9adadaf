// Stand-alone driver of the host code of tape tables (VDF_TAPE_TAB, vdf_cs_tab: vdf_amd/csrc/tape_rules.h, host/rounds_host.cpp,
// host/custom_chain_host.cpp) for the sanitizers: the recorder in all three kinds of body with its refusals (a live vdf_cs, a
// second table, dimensions past the caps), the rules with every refusal of a TAB and of a table in every mode, the five host
// evaluators over a table AT THE CAPS (4096 x 8: the last row and the last column are read) and over three rows with a counter
// that crosses 2^64 in either direction, a round body's shape against the plain loop's, and the chain constructors' copies and
// refusals.  The bodies only move table entries, so what an evaluator must write is known here byte for byte without any field
// arithmetic.  No device is touched.  tools/host_tape_table_sanitize.sh builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vdf_nova.h"

#define REQUIRE(cond)                                                                   \
  do {                                                                                  \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, vdf_nova_last_error()); return 1; } \
  } while (0)

struct Tab { const vdf_fe* table; size_t rows, cols, c0, c1; const vdf_fe* second; };

// an entry is (a, b): the produced entry is (table[J][c0], table[J][c1]) -- in either direction
static int walk_body(void* self, vdf_cs* cs, vdf_num, const vdf_num*, const vdf_num*, vdf_num* out) {
  const Tab* t = (const Tab*)self;
  out[0] = vdf_cs_tab(cs, t->table, t->rows, t->cols, t->c0);
  out[1] = vdf_cs_tab(cs, t->second ? t->second : t->table, t->rows, t->cols, t->c1);
  return 0;
}
// two variables per repetition: the two entries of row j; the carry goes on as the second
static int round_body(void* self, vdf_cs* cs, vdf_num, const vdf_num*, const vdf_num*, const vdf_num*, const vdf_num*, vdf_num* carry_out) {
  const Tab* t = (const Tab*)self;
  vdf_cs_alloc_from(cs, vdf_cs_tab(cs, t->table, t->rows, t->cols, t->c0));
  carry_out[0] = vdf_cs_alloc_from(cs, vdf_cs_tab(cs, t->second ? t->second : t->table, t->rows, t->cols, t->c1));
  return 0;
}
static int live_synthesize(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  const Tab* t = (const Tab*)self;
  z_out[0] = vdf_cs_add(cs, z_in[0], vdf_cs_tab(cs, t->table, t->rows, t->cols, 0));      // no body is being recorded: the failure flag
  return 0;
}
struct Rounds { Tab tab; uint64_t t; bool loop; };
static int circuit_synthesize(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  const Rounds* r = (const Rounds*)self;
  if (!r->loop) {
    const vdf_round_body body = {0, 1, 1, round_body, (void*)&r->tab};
    return vdf_cs_repeat(cs, &body, r->t, nullptr, z_in, nullptr, z_out) != VDF_OK;      // (only the shape is made here)
  }
  for (uint64_t j = 0; j < r->t; ++j) {
    const vdf_fe* row = r->tab.table + (j % r->tab.rows) * r->tab.cols;
    vdf_cs_alloc_from(cs, vdf_cs_const(cs, &row[r->tab.c0]));
    z_out[0] = vdf_cs_alloc_from(cs, vdf_cs_const(cs, &row[r->tab.c1]));
  }
  return 0;
}

static bool same(const vdf_fe& a, const vdf_fe& b) { return memcmp(&a, &b, sizeof(vdf_fe)) == 0; }

int main() {
  const int F = VDF_FIELD_FQ;
  const size_t R = VDF_TAPE_MAX_TAB_ROWS, Ccols = VDF_TAPE_MAX_TAB_COLS;
  // canonical elements (the top limb is 0), every one different
  std::vector<vdf_fe> big(R * Ccols), small(3 * 2);
  for (size_t r = 0; r < R; ++r)
    for (size_t c = 0; c < Ccols; ++c) big[r * Ccols + c] = vdf_fe{{r * Ccols + c + 1, r, c, 0}};
  for (size_t k = 0; k < small.size(); ++k) small[k] = vdf_fe{{100 + k, 0, 0, 0}};
  std::vector<vdf_fe> other = small;
  Tab at_caps = {big.data(), R, Ccols, 0, Ccols - 1, nullptr}, three = {small.data(), 3, 2, 0, 1, nullptr};

  static vdf_tape_op ops[3][VDF_TAPE_MAX_OPS];
  static vdf_fe consts[3][VDF_TAPE_MAX_CONSTS];
  vdf_round_tape round, walk, fwd;
  const vdf_walk_body wb = {0, 2, walk_body, &at_caps};
  const vdf_round_body rb = {0, 1, 1, round_body, &at_caps};

  // ---- the recorder ----
  REQUIRE(vdf_nova_round_body_record(F, &rb, ops[0], consts[0], &round) == VDF_OK);
  REQUIRE(vdf_nova_walk_body_record(F, &wb, ops[1], consts[1], &walk) == VDF_OK);
  REQUIRE(vdf_nova_forward_body_record(F, &wb, ops[2], consts[2], &fwd) == VDF_OK);
  for (const vdf_round_tape* tp : {&round, &walk, &fwd})
    REQUIRE(tp->table == big.data() && tp->tab_rows == R && tp->tab_cols == Ccols && tp->n_consts == 0);
  {
    Tab bad = three;
    vdf_round_tape out;
    static vdf_tape_op o2[VDF_TAPE_MAX_OPS];
    static vdf_fe c2[VDF_TAPE_MAX_CONSTS];
    const vdf_walk_body w2 = {0, 2, walk_body, &bad};
    const vdf_round_body r2 = {0, 1, 1, round_body, &bad};
    bad.second = other.data();                                     // a second table: the same elements at another address
    REQUIRE(vdf_nova_walk_body_record(F, &w2, o2, c2, &out) == VDF_ERR_BAD_ARG);
    REQUIRE(vdf_nova_forward_body_record(F, &w2, o2, c2, &out) == VDF_ERR_BAD_ARG);
    REQUIRE(vdf_nova_round_body_record(F, &r2, o2, c2, &out) == VDF_ERR_BAD_ARG);
    bad = three; bad.c1 = 2;                                       // a column past the table
    REQUIRE(vdf_nova_walk_body_record(F, &w2, o2, c2, &out) == VDF_ERR_BAD_ARG);
    bad = three; bad.rows = R + 1;
    REQUIRE(vdf_nova_walk_body_record(F, &w2, o2, c2, &out) == VDF_ERR_BAD_ARG);
    bad = three; bad.rows = 0;
    REQUIRE(vdf_nova_walk_body_record(F, &w2, o2, c2, &out) == VDF_ERR_BAD_ARG);
    bad = three; bad.cols = Ccols + 1;
    REQUIRE(vdf_nova_walk_body_record(F, &w2, o2, c2, &out) == VDF_ERR_BAD_ARG);
    bad = three; bad.table = nullptr;
    REQUIRE(vdf_nova_walk_body_record(F, &w2, o2, c2, &out) == VDF_ERR_BAD_ARG);
    bad = three;
    REQUIRE(vdf_nova_walk_body_record(F, &w2, o2, c2, &out) == VDF_OK && out.tab_rows == 3 && out.tab_cols == 2);
    // a live vdf_cs
    uint8_t digest[32];
    uint64_t sizes[2][3];
    const vdf_step_circuit live = {1, live_synthesize, &bad};
    REQUIRE(vdf_nova_shape_digest_custom(&live, VDF_GENS_TRY_AND_INCREMENT, digest, sizes) == VDF_ERR_BAD_ARG);
    // a round body with a table has the plain loop's shape and digest
    Rounds rep = {three, 7, false}, loop = {three, 7, true};
    const vdf_step_circuit c_rep = {1, circuit_synthesize, &rep}, c_loop = {1, circuit_synthesize, &loop};
    uint8_t d1[32], d2[32];
    uint64_t s1[2][3], s2[2][3];
    REQUIRE(vdf_nova_shape_digest_custom(&c_rep, VDF_GENS_TRY_AND_INCREMENT, d1, s1) == VDF_OK);
    REQUIRE(vdf_nova_shape_digest_custom(&c_loop, VDF_GENS_TRY_AND_INCREMENT, d2, s2) == VDF_OK);
    REQUIRE(memcmp(d1, d2, 32) == 0 && memcmp(s1, s2, sizeof(s1)) == 0);
  }

  // ---- the rules: every refusal, in every mode, through that mode's evaluator; nothing is written ----
  const vdf_fe guard = {{~0ull, ~0ull, ~0ull, ~0ull}};
  auto run = [&](int mode, const vdf_round_tape* tp, std::vector<vdf_fe>& buf) -> int {
    buf.assign(16, guard);
    std::vector<vdf_fe> adv(4, small[0]);
    if (mode == 0) return vdf_nova_round_tape_eval(F, tp, 1, nullptr, adv.data(), buf.data());
    if (mode == 1) return vdf_nova_walk_tape_eval(F, tp, nullptr, buf.data(), 1, 1, buf.data() + 4, 0, 1, 0, 0, 7, 0, 1, nullptr, nullptr);
    return vdf_nova_forward_tape_eval(F, tp, nullptr, buf.data(), 1, 1, buf.data() + 4, 1, 2, buf.data() + 10, 2, 0, 7, 0);
  };
  const vdf_round_tape* good[3] = {&round, &walk, &fwd};
  for (int mode = 0; mode < 3; ++mode) {
    std::vector<vdf_fe> buf;
    size_t tab_at = 0;
    while (good[mode]->ops[tab_at].op != VDF_TAPE_TAB) ++tab_at;
    for (int what = 0; what < 8; ++what) {
      std::vector<vdf_tape_op> o(good[mode]->ops, good[mode]->ops + good[mode]->n_ops);
      vdf_round_tape t = *good[mode];
      t.ops = o.data();
      switch (what) {
        case 0: t.tab_rows = t.tab_cols = 0; t.table = nullptr; break;      // a TAB in a tape without a table: opcode 11 is malformed
        case 1: o[tab_at].a = (uint8_t)Ccols; break;
        case 2: o[tab_at].b = 1; break;
        case 3: t.tab_rows = 0; break;
        case 4: t.tab_cols = 0; break;
        case 5: t.tab_rows = (uint32_t)R + 1; break;
        case 6: t.tab_cols = (uint32_t)Ccols + 1; break;
        default: t.table = nullptr; break;
      }
      REQUIRE(run(mode, &t, buf) == VDF_ERR_BAD_ARG);
      if (what == 0) REQUIRE(strstr(vdf_nova_last_error(), "malformed") != nullptr);
      for (const vdf_fe& v : buf) REQUIRE(same(v, guard));
      REQUIRE(run(mode, good[mode], buf) == VDF_OK);                // a valid call after each
    }
  }

  // ---- the five evaluators at the caps: rounds that reach the last row, and wrap to row 0 ----
  {
    const uint64_t t = R + 3;
    std::vector<vdf_fe> adv(2 * (t + 2), small[0]), out(2 * t * round.n_vars);
    REQUIRE(round.n_vars == 2);
    REQUIRE(vdf_nova_round_tape_eval(F, &round, t, nullptr, adv.data(), out.data()) == VDF_OK);
    for (uint64_t j = 0; j < t; ++j) REQUIRE(same(out[2 * j], big[(j % R) * Ccols]) && same(out[2 * j + 1], big[(j % R) * Ccols + Ccols - 1]));
    REQUIRE(vdf_nova_round_tape_eval_lanes(F, &round, t, 2, nullptr, adv.data(), t + 1, out.data()) == VDF_OK);
    for (uint64_t j = 0; j < t; ++j) REQUIRE(same(out[2 * (t + j)], big[(j % R) * Ccols]) && same(out[2 * (t + j) + 1], big[(j % R) * Ccols + Ccols - 1]));
  }
  {
    // descending from J = R + 1 to R - 2, ascending from R - 2 to R + 1: every produced entry is its round's row
    const uint64_t rounds = 4;
    std::vector<vdf_fe> e(2, small[0]), tr(2 * (rounds + 1), guard);
    REQUIRE(vdf_nova_walk_tape_eval(F, &walk, nullptr, e.data(), 1, rounds, tr.data(), 0, rounds, 0, 0, R - 2, 0, 1, nullptr, nullptr) == VDF_OK);
    for (uint64_t k = 0; k < rounds; ++k) {                         // entry k was produced under J = R - 2 + k
      const size_t row = (size_t)((R - 2 + k) % R);
      REQUIRE(same(tr[2 * k], big[row * Ccols]) && same(tr[2 * k + 1], big[row * Ccols + Ccols - 1]));
    }
    REQUIRE(same(e[0], big[(R - 2) * Ccols]));
    const uint64_t jb[2] = {R - 2, 1};
    std::vector<vdf_fe> e2(4, small[0]);
    REQUIRE(vdf_nova_walk_tape_eval_lanes(F, &walk, 2, nullptr, e2.data(), 2, rounds, nullptr, 0, rounds, 1, 0, jb, 0, 0, nullptr, nullptr) == VDF_OK);
    REQUIRE(same(e2[0], big[(R - 2) * Ccols]) && same(e2[2], big[1 * Ccols]));
    std::vector<vdf_fe> f(2, small[0]), ftr(2 * (rounds + 1), guard);
    REQUIRE(vdf_nova_forward_tape_eval(F, &fwd, nullptr, f.data(), 1, rounds, nullptr, 0, 0, ftr.data(), 0, 0, R - 2, 0) == VDF_OK);
    for (uint64_t k = 1; k <= rounds; ++k) {                        // entry k was produced under J = R - 2 + k - 1
      const size_t row = (size_t)((R - 3 + k) % R);
      REQUIRE(same(ftr[2 * k], big[row * Ccols]) && same(ftr[2 * k + 1], big[row * Ccols + Ccols - 1]));
    }
  }
  // ---- three rows and a counter that crosses 2^64: the row is (J mod 2^64) mod 3, and 2^64 is no multiple of 3 ----
  {
    vdf_round_tape w3, f3;
    static vdf_tape_op o3[2][VDF_TAPE_MAX_OPS];
    static vdf_fe c3[2][VDF_TAPE_MAX_CONSTS];
    const vdf_walk_body b3 = {0, 2, walk_body, &three};
    REQUIRE(vdf_nova_walk_body_record(F, &b3, o3[0], c3[0], &w3) == VDF_OK && vdf_nova_forward_body_record(F, &b3, o3[1], c3[1], &f3) == VDF_OK);
    const uint64_t rounds = 7, j_base = ~0ull - 4;                  // 2^64 - 5
    std::vector<vdf_fe> e(2, small[0]), tr(2 * (rounds + 1), guard);
    REQUIRE(vdf_nova_walk_tape_eval(F, &w3, nullptr, e.data(), 1, rounds, tr.data(), 0, rounds, 0, 0, j_base, 0, 1, nullptr, nullptr) == VDF_OK);
    for (uint64_t k = 0; k < rounds; ++k) REQUIRE(same(tr[2 * k], small[2 * ((uint64_t)(j_base + k) % 3)]));
    std::vector<vdf_fe> f(2, small[0]), ftr(2 * (rounds + 1), guard);
    REQUIRE(vdf_nova_forward_tape_eval(F, &f3, nullptr, f.data(), 1, rounds, nullptr, 0, 0, ftr.data(), 0, 0, j_base, 0) == VDF_OK);
    for (uint64_t k = 1; k <= rounds; ++k) REQUIRE(same(ftr[2 * k + 1], small[2 * ((uint64_t)(j_base + k - 1) % 3) + 1]));

    // ---- the chain constructors: the table is copied and counted; rows that do not divide t or a j_base are refused ----
    std::vector<vdf_fe> cps(2 * 7, small[0]);
    vdf_custom_chain* chain = nullptr;
    uint64_t bytes = 0;
    REQUIRE(vdf_nova_custom_chain_from_checkpoints(F, &w3, nullptr, 6, 3, 2, cps.data(), 3, &chain) == VDF_OK);
    REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK && bytes >= (6 + 2 * 5) * 32);
    vdf_nova_custom_chain_free(chain);
    REQUIRE(vdf_nova_custom_chain_from_checkpoints(F, &w3, nullptr, 8, 4, 1, cps.data(), 0, &chain) == VDF_ERR_BAD_ARG && !chain);
    REQUIRE(strstr(vdf_nova_last_error(), "must divide t") != nullptr);
    REQUIRE(vdf_nova_custom_chain_from_checkpoints(F, &w3, nullptr, 6, 3, 2, cps.data(), 4, &chain) == VDF_ERR_BAD_ARG && !chain);
    REQUIRE(strstr(vdf_nova_last_error(), "must divide every j_base") != nullptr);
    const uint64_t jb2[2] = {3, 5};
    REQUIRE(vdf_nova_custom_chain_lanes_from_checkpoints(F, &w3, nullptr, 6, 6, 2, 2, cps.data(), 3, jb2, &chain) == VDF_ERR_BAD_ARG && !chain);
    // the walk tape at the caps: one MiB copied
    REQUIRE(vdf_nova_custom_chain_from_checkpoints(F, &walk, nullptr, R, R, 1, cps.data(), 0, &chain) == VDF_OK);
    REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK && bytes >= R * Ccols * 32);
    vdf_nova_custom_chain_free(chain);
  }
  printf("host tape tables: ok\n");
  return 0;
}
