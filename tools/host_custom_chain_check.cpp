// Stand-alone driver of the custom chain's host code (vdf_amd/csrc/host/custom_chain_host.cpp and the seam of nova_host.cpp) for
// the sanitizers: the constructor and every refusal of it, the slicing function over the host restatement of the walk, and
// vdf_cs_step_advice while a shape is recorded.  No device is touched.  tools/host_custom_chain_sanitize.sh builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vdf_nova.h"

#define REQUIRE(cond)                                                                   \
  do {                                                                                  \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, vdf_nova_last_error()); return 1; } \
  } while (0)

// the MinRoot round backwards (examples/prove_custom_chain.c): entry j from entry j + 1
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
struct Rounds { uint64_t t; bool ask; int asked, non_null; };
static int synthesize(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  Rounds* r = (Rounds*)self;
  const vdf_round_body body = {1, 2, 2, round_body, nullptr};
  const vdf_fe* adv = nullptr;
  if (r->ask) { adv = vdf_cs_step_advice(cs); ++r->asked; r->non_null += adv != nullptr; }
  if (vdf_cs_repeat(cs, &body, r->t, &z_in[2], z_in, vdf_cs_is_witness(cs) ? adv : nullptr, z_out) != VDF_OK) return 1;
  z_out[2] = z_in[2];
  return 0;
}

int main() {
  static vdf_tape_op ops[VDF_TAPE_MAX_OPS];
  static vdf_fe consts[VDF_TAPE_MAX_CONSTS];
  const vdf_walk_body wb = {1, 2, walk_body, nullptr};
  vdf_round_tape tape;
  REQUIRE(vdf_nova_walk_body_record(VDF_FIELD_FQ, &wb, ops, consts, &tape) == VDF_OK);
  const uint64_t t = 65, every = 13;
  const size_t steps = 4, per = t / every, na = 2, n_cp = steps * per + 1;
  // a chain that is consistent by construction: its last entry is arbitrary, every entry below it is the walk's
  const vdf_fe inv = {{7, 0, 0, 0}};
  std::vector<vdf_fe> all((steps * t + 1) * na), stand(na);
  for (size_t c = 0; c < na; ++c) stand[c] = vdf_fe{{11 + c, 5, 0, 0}};
  for (size_t k = steps * t; ; --k) {
    memcpy(&all[k * na], stand.data(), na * sizeof(vdf_fe));
    if (k == 0) break;
    REQUIRE(vdf_nova_walk_tape_eval(VDF_FIELD_FQ, &tape, &inv, stand.data(), 1, 1, nullptr, 0, 0, 0, 0, k, 0, 0, nullptr, nullptr) == VDF_OK);   // (top = 0: the round sees j_base - 1)
  }
  std::vector<vdf_fe> cps(n_cp * na);
  for (size_t c = 0; c < n_cp; ++c) memcpy(&cps[c * na], &all[c * every * na], na * sizeof(vdf_fe));

  // ---- the constructor, its refusals (nothing allocated: the sanitizer's leak check sees the rest), a valid chain right after
  vdf_custom_chain* chain = (vdf_custom_chain*)1;
  auto refused = [&](int field, const vdf_round_tape* tp, const vdf_fe* iv, uint64_t tt, uint64_t ev, size_t st, const vdf_fe* cp) {
    chain = (vdf_custom_chain*)1;
    return vdf_nova_custom_chain_from_checkpoints(field, tp, iv, tt, ev, st, cp, 0, &chain) == VDF_ERR_BAD_ARG && chain == nullptr &&
           vdf_nova_last_error()[0] != 0;
  };
  REQUIRE(refused(9, &tape, &inv, t, every, steps, cps.data()));
  REQUIRE(refused(VDF_FIELD_FQ, nullptr, &inv, t, every, steps, cps.data()));
  REQUIRE(refused(VDF_FIELD_FQ, &tape, nullptr, t, every, steps, cps.data()));
  REQUIRE(refused(VDF_FIELD_FQ, &tape, &inv, t, every, steps, nullptr));
  REQUIRE(refused(VDF_FIELD_FQ, &tape, &inv, t, 0, steps, cps.data()));
  REQUIRE(refused(VDF_FIELD_FQ, &tape, &inv, t, 12, steps, cps.data()));
  REQUIRE(refused(VDF_FIELD_FQ, &tape, &inv, 0, 1, steps, cps.data()));
  REQUIRE(refused(VDF_FIELD_FQ, &tape, &inv, t, every, 0, cps.data()));
  REQUIRE(vdf_nova_custom_chain_from_checkpoints(VDF_FIELD_FQ, &tape, &inv, t, every, steps, cps.data(), 0, nullptr) == VDF_ERR_BAD_ARG);
  {
    vdf_round_tape bad = tape;
    bad.n_vars = 1;
    REQUIRE(refused(VDF_FIELD_FQ, &bad, &inv, t, every, steps, cps.data()));
    bad = tape; bad.n_slots = VDF_WALK_MAX_SLOTS;
    REQUIRE(refused(VDF_FIELD_FQ, &bad, &inv, t, every, steps, cps.data()));
    static vdf_tape_op ops2[VDF_TAPE_MAX_OPS];
    memcpy(ops2, ops, sizeof(ops));
    bad = tape; bad.ops = ops2;
    for (size_t i = 0; i < tape.n_ops; ++i) if (ops2[i].op == VDF_TAPE_ADV) { ops2[i].b = 0; break; }
    REQUIRE(refused(VDF_FIELD_FQ, &bad, &inv, t, every, steps, cps.data()));
    memcpy(ops2, ops, sizeof(ops));
    ops2[tape.n_ops - 1].op = VDF_TAPE_POW;
    REQUIRE(refused(VDF_FIELD_FQ, &bad, &inv, t, every, steps, cps.data()));
    ops2[0].op = 250;
    REQUIRE(refused(VDF_FIELD_FQ, &bad, &inv, t, every, steps, cps.data()));
  }
  REQUIRE(vdf_nova_custom_chain_from_checkpoints(VDF_FIELD_FQ, &tape, &inv, t, every, steps, cps.data(), 0, &chain) == VDF_OK && chain);
  uint64_t bytes = 0, dev_bytes = 1;
  size_t resident = 1;
  REQUIRE(vdf_nova_custom_chain_len(chain) == steps);
  REQUIRE(vdf_nova_custom_chain_host_bytes(chain, &bytes) == VDF_OK && bytes == tape.n_ops * sizeof(vdf_tape_op) + (tape.n_consts + 1 + n_cp * na) * 32);
  REQUIRE(vdf_nova_custom_chain_memory(chain, &resident, &dev_bytes) == VDF_OK && resident == 0 && dev_bytes == 0);
  REQUIRE(vdf_nova_custom_chain_materialize(nullptr, chain, 0, 1, 1, 0, nullptr) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_custom_chain_release(chain, 0, steps + 1) == VDF_ERR_BAD_LENGTH);
  REQUIRE(vdf_nova_custom_chain_release(chain, 0, steps) == VDF_OK);
  vdf_nova_custom_chain_free(chain);
  vdf_nova_custom_chain_free(nullptr);

  // ---- the slicing function: a window of steps 1 .. 3 cut into launches against one uncut call, over the host restatement
  const size_t first = 1, count = 3, walks = count * per;
  auto window = [&](uint64_t launch, std::vector<vdf_fe>& trace, std::vector<vdf_fe>& land, std::vector<int32_t>& ok) -> int {
    trace.assign(count * (t + 1) * na, vdf_fe{{~0ull, ~0ull, ~0ull, ~0ull}});
    land.assign(cps.begin() + (first * per + 1) * na, cps.begin() + (first * per + 1 + walks) * na);
    ok.assign(walks, -7);
    for (uint64_t done = 0; done < every;) {
      uint64_t now = 0, top = 0;
      int last = 0;
      if (vdf_nova_custom_chain_slice(every, launch, done, 0, &now, &top, &last) != VDF_OK || now == 0 || now > every - done) return 1;
      if (vdf_nova_walk_tape_eval(VDF_FIELD_FQ, &tape, &inv, land.data(), walks, now, trace.data(), every, top, per, t + 1, first * t, t, last,
                                  last ? &cps[first * per * na] : nullptr, last ? ok.data() : nullptr) != VDF_OK) return 1;
      done += now;
    }
    return 0;
  };
  std::vector<vdf_fe> tr1, tr2, l1, l2;
  std::vector<int32_t> ok1, ok2;
  REQUIRE(window(every, tr1, l1, ok1) == 0);
  for (uint64_t launch : {(uint64_t)4, (uint64_t)1, (uint64_t)100, (uint64_t)0}) {
    REQUIRE(window(launch, tr2, l2, ok2) == 0);
    REQUIRE(memcmp(tr1.data(), tr2.data(), tr1.size() * sizeof(vdf_fe)) == 0 && memcmp(l1.data(), l2.data(), l1.size() * sizeof(vdf_fe)) == 0 && ok1 == ok2);
  }
  for (int32_t v : ok1) REQUIRE(v == 1);
  for (size_t g = 0; g < count; ++g)               // the traces are the chain's own entries
    REQUIRE(memcmp(&tr1[g * (t + 1) * na], &all[(first + g) * t * na], (t + 1) * na * sizeof(vdf_fe)) == 0);
  uint64_t now, top;
  int last;
  REQUIRE(vdf_nova_custom_chain_slice(0, 4, 0, 0, &now, &top, &last) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_custom_chain_slice(13, 4, 13, 0, &now, &top, &last) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_custom_chain_slice(13, 4, 0, 0, nullptr, &top, &last) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_custom_chain_slice(13, 4, 8, 3, &now, &top, &last) == VDF_OK && now == 3 && top == 5 && last == 0);

  // ---- vdf_cs_step_advice while a shape is recorded: NULL, and the digest of the circuit that asks is the one of the circuit that does not
  Rounds asks = {5, true, 0, 0}, plain = {5, false, 0, 0};
  const vdf_step_circuit c1 = {3, synthesize, &asks}, c2 = {3, synthesize, &plain};
  uint8_t d1[32], d2[32];
  uint64_t s1[2][3], s2[2][3];
  REQUIRE(vdf_nova_shape_digest_custom(&c1, VDF_GENS_TRY_AND_INCREMENT, d1, s1) == VDF_OK);
  REQUIRE(vdf_nova_shape_digest_custom(&c2, VDF_GENS_TRY_AND_INCREMENT, d2, s2) == VDF_OK);
  REQUIRE(asks.asked > 0 && asks.non_null == 0 && memcmp(d1, d2, 32) == 0 && memcmp(s1, s2, sizeof(s1)) == 0);
  REQUIRE(vdf_cs_step_advice(nullptr) == nullptr);
  printf("host custom chain check: ok\n");
  return 0;
}
