/* A custom step circuit whose rounds run on the GPU, in plain C: the forward MinRoot round written through the step-circuit
 * seam (vdf_step_circuit + vdf_cs_repeat) instead of taken from the library's built-in kinds.
 *
 *   the round, once, as a callback over the vdf_cs_* calls              round_body (recorded into a tape by vdf_cs_repeat)
 *   the step circuit around it: t repetitions, z = (x, y, i)            synthesize
 *   parameters of that circuit                                          vdf_nova_public_params_custom
 *   evaluation (host), the step's trace into device memory as advice    vdf_minroot_eval, vdf_dev_memcpy
 *   one prove_step per trace: the rounds' variables are made by a kernel vdf_nova_prove_step_custom
 *   verification: z0 = the initial state, zi = the final one            vdf_nova_verify_custom
 *
 * Any other uniform round (another exponent, another round shape) is a change of round_body alone.
 * Build:  cc -O2 examples/prove_custom_rounds.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/prove_custom_rounds
 * Run:    examples/prove_custom_rounds [iterations per step = 65] [steps = 3] [x0 = 123] [bench]
 *         It prints the parameters' digest (a 250-bit integer, hexadecimal).  With `bench` it then times the same chain three
 *         times over, alternating between this circuit and the same circuit written as a plain loop of vdf_cs_* calls (one
 *         host callback per multiplication, the whole witness uploaded: what the seam costs without vdf_cs_repeat), and
 *         prints the milliseconds per step of every run (tools/gpu_custom_rounds.py reads them).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "vdf_nova.h"

#define CHECK(expr, what)                                                                                         \
  do {                                                                                                              \
    int rc_ = (expr);                                                                                               \
    if (rc_ != VDF_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc_, vdf_nova_last_error()); return 1; }   \
  } while (0)

typedef struct { uint64_t t; const vdf_fe* advice; } rounds;      /* advice: this step's trace (device memory); NULL for the shape */
static double now_ms(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

/* x' = the fifth root of x + y, taken from the next entry of the trace and bound by x'^5 = x + y; y' = x + i_in + j */
static int round_body(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* carry, const vdf_num* cur, const vdf_num* next,
                      vdf_num* carry_out) {
  (void)self; (void)cur;
  const vdf_num xn = vdf_cs_alloc_from(cs, next[0]);
  const vdf_num t1 = vdf_cs_mul(cs, xn, xn);
  const vdf_num t2 = vdf_cs_mul(cs, t1, t1);
  if (vdf_cs_enforce(cs, t2, xn, vdf_cs_add(cs, carry[0], carry[1])) != VDF_OK) return 1;
  carry_out[0] = xn;
  carry_out[1] = vdf_cs_add(cs, vdf_cs_add(cs, carry[0], inv[0]), j);
  return 0;
}

static int synthesize(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  const rounds* r = (const rounds*)self;
  const vdf_round_body body = {1, 2, 2, round_body, NULL};
  vdf_fe tt;
  if (vdf_minroot_element(VDF_FIELD_FQ, r->t, &tt) != VDF_OK) return 1;
  if (vdf_cs_repeat(cs, &body, r->t, &z_in[2], z_in, vdf_cs_is_witness(cs) ? r->advice : NULL, z_out) != VDF_OK) return 1;
  z_out[2] = vdf_cs_add(cs, z_in[2], vdf_cs_const(cs, &tt));
  return 0;
}

/* the same circuit without vdf_cs_repeat (bench only): the calls of round_body t times over, the roots allocated from the HOST trace */
static int synthesize_plain(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  const rounds* r = (const rounds*)self;
  const int wit = vdf_cs_is_witness(cs);
  vdf_num x = z_in[0], y = z_in[1];
  vdf_fe k;
  for (uint64_t j = 0; j < r->t; ++j) {
    const vdf_num xn = vdf_cs_alloc(cs, wit ? &r->advice[2 * (j + 1)] : NULL);
    const vdf_num t1 = vdf_cs_mul(cs, xn, xn);
    const vdf_num t2 = vdf_cs_mul(cs, t1, t1);
    if (vdf_cs_enforce(cs, t2, xn, vdf_cs_add(cs, x, y)) != VDF_OK) return 1;
    if (vdf_minroot_element(VDF_FIELD_FQ, j, &k) != VDF_OK) return 1;
    y = vdf_cs_add(cs, vdf_cs_add(cs, x, z_in[2]), vdf_cs_const(cs, &k));
    x = xn;
  }
  if (vdf_minroot_element(VDF_FIELD_FQ, r->t, &k) != VDF_OK) return 1;
  z_out[0] = x; z_out[1] = y;
  z_out[2] = vdf_cs_add(cs, z_in[2], vdf_cs_const(cs, &k));
  return 0;
}

/* `steps` steps of one form over traces kept by the caller; *ms_per_step = wall time of the steps alone */
static int timed_chain(vdf_ctx* ctx, vdf_pp* pp, const vdf_step_circuit* circuit, rounds* r, vdf_fe* const* advice, size_t steps, const vdf_fe* z0,
                       const vdf_fe* zi, double* ms_per_step) {
  vdf_proof* proof = NULL;
  int ok = 0;
  const double t0 = now_ms();
  for (size_t k = 0; k < steps; ++k) {
    r->advice = advice[k];
    CHECK(vdf_nova_prove_step_custom(pp, &proof, circuit, z0), "prove_step_custom");
  }
  CHECK(vdf_ctx_sync(ctx), "ctx_sync");
  *ms_per_step = (now_ms() - t0) / (double)steps;
  CHECK(vdf_nova_verify_custom(proof, pp, steps, z0, zi, &ok), "verify_custom");
  vdf_nova_proof_free(proof);
  return ok ? 0 : 1;
}

int main(int argc, char** argv) {
  const uint64_t t = argc > 1 ? strtoull(argv[1], NULL, 10) : 65;
  const size_t steps = argc > 2 ? (size_t)atoi(argv[2]) : 3;
  const uint64_t x0 = argc > 3 ? strtoull(argv[3], NULL, 10) : 123;
  const int bench = argc > 4 && strcmp(argv[4], "bench") == 0;
  if (t < 1 || t > (1u << 20) || steps < 1 || steps > 1000) { fprintf(stderr, "usage: prove_custom_rounds [t] [steps] [x0] [bench]\n"); return 2; }

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  rounds r = {t, NULL};
  const vdf_step_circuit circuit = {3, synthesize, &r};
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params_custom(ctx, &circuit, VDF_GENS_TRY_AND_INCREMENT, &pp), "public_params_custom");
  uint8_t digest[32];
  uint64_t seg_begin = 0, seg_len = 0;
  CHECK(vdf_nova_pp_digest(pp, digest), "pp_digest");
  CHECK(vdf_nova_pp_segment(pp, &seg_begin, &seg_len), "pp_segment");
  printf("digest: ");
  for (int k = 31; k >= 0; --k) printf("%02x", digest[k]);
  printf("\nrounds on the device: %llu variables from %llu\n", (unsigned long long)seg_len, (unsigned long long)seg_begin);

  vdf_state s, next;
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, x0, &s.x), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &s.y), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &s.i), "element");
  const vdf_fe z0[3] = {s.x, s.y, s.i};

  const size_t trace_bytes = (size_t)(t + 1) * 2 * sizeof(vdf_fe);
  vdf_fe* trace = (vdf_fe*)malloc(trace_bytes);
  void* d_trace = NULL;
  if (!trace) return 1;
  CHECK(vdf_dev_alloc(ctx, trace_bytes, &d_trace), "dev_alloc");
  vdf_proof* proof = NULL;
  for (size_t k = 0; k < steps; ++k) {
    CHECK(vdf_minroot_eval(VDF_FIELD_FQ, VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL, &s, t, &next, trace), "eval");
    CHECK(vdf_dev_memcpy(ctx, d_trace, trace, trace_bytes), "dev_memcpy");
    r.advice = (const vdf_fe*)d_trace;
    CHECK(vdf_nova_prove_step_custom(pp, &proof, &circuit, z0), "prove_step_custom");
    s = next;
  }
  const vdf_fe zi[3] = {s.x, s.y, s.i};
  int ok = 0, all_ok;
  CHECK(vdf_nova_verify_custom(proof, pp, steps, z0, zi, &ok), "verify_custom");
  printf("verify: %s\n", ok ? "true" : "FALSE");
  all_ok = ok;
  CHECK(vdf_nova_verify_custom(proof, pp, steps, zi, z0, &ok), "verify_custom (swapped)");
  printf("verify with z0 and zi swapped: %s\n", ok ? "TRUE" : "false");
  all_ok = all_ok && !ok;

  vdf_nova_proof_free(proof);
  vdf_dev_free(ctx, d_trace);
  free(trace);

  if (bench && all_ok) {
    /* every step's trace on the host (the plain loop allocates from it) and on the device (the repeat's advice), made up front */
    vdf_fe** h_tr = (vdf_fe**)calloc(steps, sizeof(vdf_fe*));
    vdf_fe** d_tr = (vdf_fe**)calloc(steps, sizeof(vdf_fe*));
    vdf_state b = {z0[0], z0[1], z0[2]};
    if (!h_tr || !d_tr) return 1;
    for (size_t k = 0; k < steps; ++k) {
      void* d = NULL;
      h_tr[k] = (vdf_fe*)malloc(trace_bytes);
      if (!h_tr[k]) return 1;
      CHECK(vdf_minroot_eval(VDF_FIELD_FQ, VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL, &b, t, &next, h_tr[k]), "eval");
      CHECK(vdf_dev_alloc(ctx, trace_bytes, &d), "dev_alloc");
      CHECK(vdf_dev_memcpy(ctx, d, h_tr[k], trace_bytes), "dev_memcpy");
      d_tr[k] = (vdf_fe*)d;
      b = next;
    }
    rounds rp = {t, NULL};
    const vdf_step_circuit plain = {3, synthesize_plain, &rp};
    vdf_pp* pp_plain = NULL;
    uint8_t digest_plain[32];
    CHECK(vdf_nova_public_params_custom(ctx, &plain, VDF_GENS_TRY_AND_INCREMENT, &pp_plain), "public_params_custom (plain loop)");
    CHECK(vdf_nova_pp_digest(pp_plain, digest_plain), "pp_digest");
    printf("plain loop has the same digest: %s\n", memcmp(digest, digest_plain, 32) == 0 ? "true" : "FALSE");
    for (int run = 0; run < 4 && all_ok; ++run) {            /* run 0 warms both forms up */
      double ms_dev = 0, ms_plain = 0;
      all_ok = timed_chain(ctx, pp, &circuit, &r, d_tr, steps, z0, zi, &ms_dev) == 0 &&
               timed_chain(ctx, pp_plain, &plain, &rp, h_tr, steps, z0, zi, &ms_plain) == 0;
      if (run) printf("bench run %d: repeat on the device %.4f ms per step, plain loop %.4f ms per step\n", run, ms_dev, ms_plain);
    }
    for (size_t k = 0; k < steps; ++k) { free(h_tr[k]); vdf_dev_free(ctx, d_tr[k]); }
    free(h_tr); free(d_tr);
    vdf_nova_pp_free(pp_plain);
  }
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return all_ok ? 0 : 1;
}
