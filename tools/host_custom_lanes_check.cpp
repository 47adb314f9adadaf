// Stand-alone driver of the host code of custom chains in lanes (vdf_amd/csrc/host/custom_chain_host.cpp, rounds_host.cpp and the
// seam of nova_host.cpp) for the sanitizers: the lanes constructor and every refusal of it, the host restatement of the lanes walk
// against `lanes` single walks over the same trace, the host restatement of the rounds in lanes against the single one, and
// vdf_cs_repeat_lanes while a shape is recorded, with its refusals.  No device is touched.  tools/host_custom_lanes_sanitize.sh
// builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vdf_nova.h"

#define REQUIRE(cond)                                                                   \
  do {                                                                                  \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, vdf_nova_last_error()); return 1; } \
  } while (0)

// the MinRoot round backwards (examples/prove_custom_lanes.c): entry j from entry j + 1
static int walk_body(void*, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* next, vdf_num* cur_out) {
  const vdf_num x = vdf_cs_sub(cs, next[1], vdf_cs_add(cs, inv[0], j));
  const vdf_num x2 = vdf_cs_mul(cs, next[0], next[0]);
  cur_out[0] = x;
  cur_out[1] = vdf_cs_sub(cs, vdf_cs_mul(cs, vdf_cs_mul(cs, x2, x2), next[0]), x);
  return 0;
}
static int round_body(void*, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* carry, const vdf_num*, const vdf_num* next, vdf_num* out) {
  const vdf_num xn = vdf_cs_alloc_from(cs, next[0]);
  const vdf_num t1 = vdf_cs_mul(cs, xn, xn);
  if (vdf_cs_enforce(cs, vdf_cs_mul(cs, t1, t1), xn, vdf_cs_add(cs, carry[0], carry[1])) != VDF_OK) return 1;
  out[0] = xn;
  out[1] = vdf_cs_add(cs, vdf_cs_add(cs, carry[0], inv[0]), j);
  return 0;
}
// arity 3 * arity_lanes; `lanes` is what the repeat is asked for (the refusals ask for more handles than z has: they are repeated)
struct Lanes { uint64_t t; size_t arity_lanes, lanes, stride; };
static int synthesize(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  const Lanes* r = (const Lanes*)self;
  const vdf_round_body body = {1, 2, 2, round_body, nullptr};
  vdf_num inv[VDF_TAPE_MAX_LANES + 1], carry[2 * VDF_TAPE_MAX_LANES + 2], out[2 * VDF_TAPE_MAX_LANES + 2];
  for (size_t l = 0; l <= VDF_TAPE_MAX_LANES; ++l) {
    const size_t at = 3 * (l % r->arity_lanes);
    carry[2 * l] = z_in[at]; carry[2 * l + 1] = z_in[at + 1]; inv[l] = z_in[at + 2];
  }
  if (vdf_cs_repeat_lanes(cs, &body, r->t, r->lanes, inv, carry, nullptr, r->stride, out) != VDF_OK) return 1;
  for (size_t l = 0; l < r->arity_lanes; ++l) { z_out[3 * l] = out[2 * l]; z_out[3 * l + 1] = out[2 * l + 1]; z_out[3 * l + 2] = z_in[3 * l + 2]; }
  return 0;
}
static int digest_of(Lanes* r, uint8_t d[32]) {
  const vdf_step_circuit c = {3 * r->arity_lanes, synthesize, r};
  uint64_t sizes[2][3];
  return vdf_nova_shape_digest_custom(&c, VDF_GENS_TRY_AND_INCREMENT, d, sizes);
}

int main() {
  const int F = VDF_FIELD_FQ;
  static vdf_tape_op w_ops[VDF_TAPE_MAX_OPS], r_ops[VDF_TAPE_MAX_OPS];
  static vdf_fe w_consts[VDF_TAPE_MAX_CONSTS], r_consts[VDF_TAPE_MAX_CONSTS];
  const vdf_walk_body wb = {1, 2, walk_body, nullptr};
  const vdf_round_body rb = {1, 2, 2, round_body, nullptr};
  vdf_round_tape walk, round;
  REQUIRE(vdf_nova_walk_body_record(F, &wb, w_ops, w_consts, &walk) == VDF_OK);
  REQUIRE(vdf_nova_round_body_record(F, &rb, r_ops, r_consts, &round) == VDF_OK);

  // ---- the lanes walk on the host against `lanes` single walks over the same trace ----
  const size_t lanes = 5, steps = 3, t = 10, every = 5, per = t / every, n = steps * lanes * per, na = 2;
  std::vector<vdf_fe> inv(lanes), start(n * na), trace(steps * lanes * (t + 1) * na + na), trace2(trace.size());
  uint64_t j_base[VDF_TAPE_MAX_LANES];
  for (size_t l = 0; l < lanes; ++l) { inv[l] = vdf_fe{{100 + l, l, 0, 0}}; j_base[l] = l == 1 ? ~0ull - 11 : 1000 * l; }
  for (size_t k = 0; k < start.size(); ++k) start[k] = vdf_fe{{3 * k + 1, k * k, 7, 0}};
  memset(trace.data(), 0xff, trace.size() * 32);
  memset(trace2.data(), 0xff, trace2.size() * 32);
  std::vector<vdf_fe> e1 = start, e2 = start;
  std::vector<int32_t> ok1(n, -7), ok2(n, -7);
  REQUIRE(vdf_nova_walk_tape_eval_lanes(F, &walk, lanes, inv.data(), e1.data(), n, every, trace.data(), every, every, per, t + 1, j_base, t, 1,
                                        start.data(), ok1.data()) == VDF_OK);
  for (size_t l = 0; l < lanes; ++l) {
    std::vector<vdf_fe> mine, expect;
    std::vector<size_t> at;
    for (size_t w = 0; w < n; ++w)
      if ((w / per) % lanes == l) { at.push_back(w); for (size_t c = 0; c < na; ++c) { mine.push_back(start[w * na + c]); expect.push_back(start[w * na + c]); } }
    std::vector<int32_t> ok(at.size(), -7);
    REQUIRE(vdf_nova_walk_tape_eval(F, &walk, &inv[l], mine.data(), at.size(), every, trace2.data() + l * (t + 1) * na, every, every, per,
                                    lanes * (t + 1), j_base[l], t, 1, expect.data(), ok.data()) == VDF_OK);
    for (size_t q = 0; q < at.size(); ++q) { memcpy(&e2[at[q] * na], &mine[q * na], na * 32); ok2[at[q]] = ok[q]; }
  }
  REQUIRE(memcmp(e1.data(), e2.data(), e1.size() * 32) == 0 && memcmp(trace.data(), trace2.data(), trace.size() * 32) == 0 && ok1 == ok2);
  for (size_t c = 0; c < 4 * na; ++c) REQUIRE(((const uint64_t*)&trace[trace.size() - na])[c] == ~0ull);      // the guard entry behind the window
  // refusals, each with nothing written
  std::vector<vdf_fe> e3 = start;
  REQUIRE(vdf_nova_walk_tape_eval_lanes(F, &walk, 0, inv.data(), e3.data(), n, every, nullptr, every, every, per, t + 1, j_base, t, 0, nullptr, nullptr) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_walk_tape_eval_lanes(F, &walk, 17, inv.data(), e3.data(), n, every, nullptr, every, every, per, t + 1, j_base, t, 0, nullptr, nullptr) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_walk_tape_eval_lanes(F, &walk, lanes, inv.data(), e3.data(), n, every, nullptr, every, every, per, t + 1, nullptr, t, 0, nullptr, nullptr) == VDF_ERR_BAD_ARG);
  REQUIRE(memcmp(e3.data(), start.data(), e3.size() * 32) == 0);

  // ---- the rounds in lanes on the host against lane after lane ----
  {
    const size_t stride = t + 3;
    std::vector<vdf_fe> adv((lanes - 1) * stride * na + (t + 1) * na), out(lanes * t * round.n_vars), one(t * round.n_vars);
    for (size_t k = 0; k < adv.size(); ++k) adv[k] = vdf_fe{{k + 1, 5 * k, 0, 1}};
    REQUIRE(vdf_nova_round_tape_eval_lanes(F, &round, t, lanes, inv.data(), adv.data(), stride, out.data()) == VDF_OK);
    for (size_t l = 0; l < lanes; ++l) {
      REQUIRE(vdf_nova_round_tape_eval(F, &round, t, &inv[l], adv.data() + l * stride * na, one.data()) == VDF_OK);
      REQUIRE(memcmp(one.data(), out.data() + l * t * round.n_vars, one.size() * 32) == 0);
    }
    REQUIRE(vdf_nova_round_tape_eval_lanes(F, &round, t, lanes, inv.data(), adv.data(), t, out.data()) == VDF_ERR_BAD_ARG);
    REQUIRE(vdf_nova_round_tape_eval_lanes(F, &round, t, 0, inv.data(), adv.data(), stride, out.data()) == VDF_ERR_BAD_ARG);
    REQUIRE(vdf_nova_round_tape_eval_lanes(F, &round, t, 17, inv.data(), adv.data(), stride, out.data()) == VDF_ERR_BAD_ARG);
  }

  // ---- the constructor and its refusals ----
  {
    const size_t per_lane = steps * per + 1, stride = per_lane + 2;
    std::vector<vdf_fe> cps(((lanes - 1) * stride + per_lane) * na);
    for (size_t k = 0; k < cps.size(); ++k) cps[k] = vdf_fe{{k, 1, 2, 3}};
    vdf_custom_chain* chain = (vdf_custom_chain*)1;
    auto make = [&](size_t L, size_t st, const uint64_t* jb, const vdf_fe* iv, uint64_t ev) {
      return vdf_nova_custom_chain_lanes_from_checkpoints(F, &walk, iv, t, ev, steps, L, cps.data(), st, jb, &chain);
    };
    REQUIRE(make(0, stride, j_base, inv.data(), every) == VDF_ERR_BAD_ARG && chain == nullptr);
    REQUIRE(make(17, stride, j_base, inv.data(), every) == VDF_ERR_BAD_ARG && chain == nullptr);
    REQUIRE(make(lanes, per_lane - 1, j_base, inv.data(), every) == VDF_ERR_BAD_ARG && chain == nullptr);
    REQUIRE(make(lanes, stride, nullptr, inv.data(), every) == VDF_ERR_BAD_ARG && chain == nullptr);
    REQUIRE(make(lanes, stride, j_base, nullptr, every) == VDF_ERR_BAD_ARG && chain == nullptr);
    REQUIRE(make(lanes, stride, j_base, inv.data(), 3) == VDF_ERR_BAD_ARG && chain == nullptr);
    REQUIRE(make(lanes, stride, j_base, inv.data(), every) == VDF_OK && chain != nullptr);
    uint64_t bytes = 0;
    REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK);
    REQUIRE(bytes == walk.n_ops * sizeof(vdf_tape_op) + walk.n_consts * 32 + lanes * walk.n_inv * 32 + lanes * per_lane * na * 32);
    REQUIRE(vdf_nova_custom_chain_len(chain) == steps);
    const vdf_fe* adv = (const vdf_fe*)1;
    REQUIRE(vdf_nova_custom_chain_advice(chain, 1, &adv) == VDF_OK && adv == nullptr);
    vdf_nova_custom_chain_free(chain);
    // one lane through the constructor that was there
    REQUIRE(vdf_nova_custom_chain_from_checkpoints(F, &walk, inv.data(), t, every, steps, cps.data(), 5, &chain) == VDF_OK);
    REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK);
    REQUIRE(bytes == walk.n_ops * sizeof(vdf_tape_op) + walk.n_consts * 32 + walk.n_inv * 32 + per_lane * na * 32);
    vdf_nova_custom_chain_free(chain);
  }

  // ---- vdf_cs_repeat_lanes in shape mode ----
  {
    uint8_t d1[32], d2[32], d3[32];
    Lanes a = {t, 3, 3, t + 1}, wide = {t, 3, 3, t + 9}, two = {t, 2, 2, t + 1};
    REQUIRE(digest_of(&a, d1) == VDF_OK && digest_of(&wide, d2) == VDF_OK && digest_of(&two, d3) == VDF_OK);
    REQUIRE(memcmp(d1, d2, 32) == 0 && memcmp(d1, d3, 32) != 0);
    Lanes none = {t, 2, 0, t + 1}, many = {t, 2, VDF_TAPE_MAX_LANES + 1, t + 1}, narrow = {t, 2, 2, t};
    REQUIRE(digest_of(&none, d2) != VDF_OK && digest_of(&many, d2) != VDF_OK && digest_of(&narrow, d2) != VDF_OK);
    Lanes full = {2, VDF_TAPE_MAX_LANES, VDF_TAPE_MAX_LANES, 3};
    REQUIRE(digest_of(&full, d2) == VDF_OK);
    REQUIRE(digest_of(&a, d2) == VDF_OK && memcmp(d1, d2, 32) == 0);
  }
  printf("host_custom_lanes_check: ok\n");
  return 0;
}
