// Stand-alone driver of the host code behind tuning.custom_ahead (vdf_amd/csrc/host/nova_host.cpp, rounds_host.cpp) for the
// sanitizers: the tuning field and its reading, the generalised early-row rule through vdf_nova_shape_early_rows_custom on circuit F
// (and on a variant with a variable between z_in and the repeat, and one whose inv is a variable of its own), and the PROBE mode of
// vdf_cs_repeat, which needs no device: its advice pointer is a host address no device call could accept, poisoned for the
// sanitizer's sake, and never looked at.  No device is touched.  tools/host_custom_ahead_sanitize.sh builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../vdf_amd/csrc/host/nova_internal.hpp"

#define REQUIRE(cond)                                                                   \
  do {                                                                                  \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, vdf_nova_last_error()); return 1; } \
  } while (0)

static int round_body(void*, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* carry, const vdf_num*, const vdf_num* next, vdf_num* out) {
  const vdf_num xn = vdf_cs_alloc_from(cs, next[0]);
  const vdf_num t1 = vdf_cs_mul(cs, xn, xn);
  if (vdf_cs_enforce(cs, vdf_cs_mul(cs, t1, t1), xn, vdf_cs_add(cs, carry[0], carry[1])) != VDF_OK) return 1;
  out[0] = xn;
  out[1] = vdf_cs_add(cs, vdf_cs_add(cs, carry[0], inv[0]), j);
  return 0;
}
// circuit F over the step's advice; gap: a variable of its own in front of the repeat; own: inv is a variable of its own
struct Rounds { uint64_t t; bool gap, own; int probes, calls; vdf_fe carry_seen[2]; };
static int synthesize(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  Rounds* r = (Rounds*)self;
  ++r->calls;
  r->probes += vdf_cs_is_probe(cs);
  const vdf_round_body body = {1, 2, 2, round_body, nullptr};
  const vdf_fe five = {{5, 0, 0, 0}};
  if (r->gap) vdf_cs_alloc(cs, &five);
  vdf_num inv = z_in[2];
  if (r->own) {
    vdf_fe v = {{0, 0, 0, 0}};
    if (vdf_cs_is_witness(cs) && vdf_cs_value(cs, z_in[2], &v) != VDF_OK) return 1;
    inv = vdf_cs_alloc(cs, &v);
  }
  if (vdf_cs_repeat(cs, &body, r->t, &inv, z_in, vdf_cs_is_witness(cs) ? vdf_cs_step_advice(cs) : nullptr, z_out) != VDF_OK) return 1;
  if (vdf_cs_is_witness(cs) && (vdf_cs_value(cs, z_out[0], &r->carry_seen[0]) != VDF_OK || vdf_cs_value(cs, z_out[1], &r->carry_seen[1]) != VDF_OK)) return 1;
  z_out[2] = z_in[2];
  return 0;
}

int main() {
  // ---- the tuning field
  vdf_nova_tuning d, got;
  vdf_nova_tuning_default(&d);
  REQUIRE(d.custom_ahead == 0 && d.struct_size == sizeof(vdf_nova_tuning));
  REQUIRE(vdf_nova_tuning_read(nullptr, &got) == VDF_OK && got.custom_ahead == 0);
  d.custom_ahead = 2;
  REQUIRE(vdf_nova_tuning_read(&d, &got) == VDF_OK && got.custom_ahead == 2);
  {
    // a caller compiled before the field: its struct ends where custom_ahead begins, and nothing behind it may be read
    const size_t old = offsetof(vdf_nova_tuning, custom_ahead);
    std::vector<unsigned char> small(old);
    memcpy(small.data(), &d, old);
    const uint32_t sz = (uint32_t)old;
    memcpy(small.data(), &sz, 4);
    REQUIRE(vdf_nova_tuning_read((const vdf_nova_tuning*)small.data(), &got) == VDF_OK && got.custom_ahead == 0 && got.periodic_rows == d.periodic_rows &&
            got.struct_size == sizeof(vdf_nova_tuning));
  }
  d.custom_ahead = 3;
  REQUIRE(vdf_nova_tuning_read(&d, &got) == VDF_ERR_BAD_ARG);
  d.custom_ahead = 1; d.struct_size = 12;
  REQUIRE(vdf_nova_tuning_read(&d, &got) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_nova_tuning_read(&d, nullptr) == VDF_ERR_BAD_ARG);

  // ---- which rows are early: F at t = 65 and t = 5, in both fields; the two variants
  for (int field : {VDF_FIELD_FQ, VDF_FIELD_FP}) {
    Rounds f65 = {65, false, false, 0, 0, {}}, f5 = {5, false, false, 0, 0, {}}, gap = {65, true, false, 0, 0, {}}, own = {65, false, true, 0, 0, {}};
    const vdf_step_circuit c65 = {3, synthesize, &f65}, c5 = {3, synthesize, &f5}, cgap = {3, synthesize, &gap}, cown = {3, synthesize, &own};
    uint64_t rb = 9, n = 9, zin = 9, seg = 9, rb2 = 9, n2 = 9, zin2 = 9, seg2 = 9;
    REQUIRE(vdf_nova_shape_early_rows_custom(field, &c65, &rb, &n, &zin, &seg) == VDF_OK);
    REQUIRE(n == 3 * 65 && seg == zin + 3 && rb > 0);
    REQUIRE(vdf_nova_shape_early_rows_custom(field, &cgap, &rb2, &n2, &zin2, &seg2) == VDF_OK);
    REQUIRE(rb2 == rb && n2 == n && zin2 == zin && seg2 == seg + 1);
    REQUIRE(vdf_nova_shape_early_rows_custom(field, &c5, &rb2, &n2, &zin2, &seg2) == VDF_OK);
    REQUIRE(rb2 == 0 && n2 == 0 && zin2 == zin && seg2 == seg);
    REQUIRE(vdf_nova_shape_early_rows_custom(field, &cown, &rb2, &n2, &zin2, &seg2) == VDF_OK);
    REQUIRE(rb2 == 0 && n2 == 0 && zin2 == zin && seg2 == seg + 1);
    REQUIRE(vdf_nova_shape_early_rows_custom(field, &c65, nullptr, nullptr, nullptr, nullptr) == VDF_OK);
    REQUIRE(f65.probes == 0 && f65.calls > 0);           // a shape synthesis is no probe
  }
  REQUIRE(vdf_nova_shape_early_rows_custom(7, nullptr, nullptr, nullptr, nullptr, nullptr) == VDF_ERR_BAD_ARG);
  REQUIRE(vdf_cs_is_probe(nullptr) == 0);

  // ---- the probe: a witness-mode synthesis whose vdf_cs_repeat records the body, keeps inv, returns zero carries, makes no
  // variable and no row, and looks at nothing of the advice -- here a host buffer no device call would take, with no device context
  {
    using namespace vdfnova;
    const uint64_t t = 65;
    Rounds r = {t, true, false, 0, 0, {}};
    const vdf_step_circuit c = {3, synthesize, &r};
    std::vector<vdf_fe> trace(2 * (t + 1), vdf_fe{{~0ull, ~0ull, ~0ull, ~0ull}});      // (not even field elements)
    std::unique_ptr<StepCircuit> probe = make_custom_circuit(&c, nullptr, trace.data(), trace.size(), true);
    CS cs(VDF_FIELD_FQ, false);
    std::vector<Num> z(3, cs.zero_num());
    const Field& F = field(VDF_FIELD_FQ);
    for (int k = 0; k < 3; ++k) z[k].v = from_u64(100 + k, F);
    const std::vector<Num> out = probe->synthesize(cs, z);
    REQUIRE(r.calls == 1 && r.probes == 1 && out.size() == 3);
    REQUIRE(cs.W.size() == 1 && cs.dev_len == 0 && cs.rows == 0);                        // the circuit's own variable, nothing of the repeat
    REQUIRE(out[0].v.is_zero() && out[1].v.is_zero() && out[2].v == z[2].v);
    vdf_fe zero_fe = {{0, 0, 0, 0}};
    REQUIRE(memcmp(&r.carry_seen[0], &zero_fe, 32) == 0 && memcmp(&r.carry_seen[1], &zero_fe, 32) == 0);
    // a repeat that would read past the step's trace is refused in a probe too, before anything is recorded
    Rounds big = {t + 1, false, false, 0, 0, {}};
    const vdf_step_circuit cbig = {3, synthesize, &big};
    std::unique_ptr<StepCircuit> probe2 = make_custom_circuit(&cbig, nullptr, trace.data(), trace.size(), true);
    CS cs2(VDF_FIELD_FQ, false);
    probe2->synthesize(cs2, z);
    REQUIRE(big.calls == 1 && cs2.W.empty() && strstr(vdf_nova_last_error(), "reads past the step's trace") != nullptr);
    // outside a probe the same host buffer is host advice: the tape is interpreted, 3 t variables are made
    Rounds plain = {t, false, false, 0, 0, {}};
    const vdf_step_circuit cp = {3, synthesize, &plain};
    for (vdf_fe& e : trace) e = vdf_fe{{3, 0, 0, 0}};
    std::unique_ptr<StepCircuit> real = make_custom_circuit(&cp, nullptr, trace.data(), trace.size(), false);
    CS cs3(VDF_FIELD_FQ, false);
    real->synthesize(cs3, z);
    REQUIRE(plain.probes == 0 && cs3.W.size() == 3 * t);
  }
  printf("host custom ahead check: ok\n");
  return 0;
}
