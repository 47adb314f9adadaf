/* Many MinRoot chains evaluated on the GPU, and two of them proved, in plain C: no Python, no torch, no HIP headers.
 *
 *   N chains evaluated at once, one lane each, a state kept every `every` rounds      vdf_minroot_eval_batch
 *   every interval of every chain checked by an inverse walk (the reference's check)  vdf_minroot_check_batch
 *   the first and the last chain proved from those checkpoints, forward circuit:      vdf_nova_circuits_forward_begin
 *     one step per t rounds from its t / every + 1 states                             vdf_nova_circuits_push_checkpoints
 *     traces rebuilt on the GPU by inverse walks                                      vdf_nova_circuits_materialize
 *     one fold per step                                                               vdf_nova_prove_step
 *   verification of each running proof: z0 = the chain's initial state, zi = final    vdf_nova_verify
 *
 * This is a THROUGHPUT arrangement: the device evaluates thousands of chains in the time a host core evaluates a few, but a
 * single chain advances far more slowly on a lane than on a core.  It is not a faster VDF.
 * Build:  cc -O2 examples/eval_farm.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/eval_farm
 * Run:    examples/eval_farm [chains = 256] [log2 iterations per step = 10] [steps = 4] [log2 every = log2 t - 2]
 *         One line per chain; exit status 0 iff every interval checked, both proofs verified and the two proved chains end
 *         where vdf_minroot_eval (host) ends.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "vdf_nova.h"

static double now_ms(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

#define CHECK(expr, what)                                                                                         \
  do {                                                                                                              \
    int rc_ = (expr);                                                                                               \
    if (rc_ != VDF_OK) {                                                                                            \
      fprintf(stderr, "%s failed (%d): %s | %s\n", what, rc_, vdf_nova_last_error(), vdf_last_error(ctx));         \
      return 1;                                                                                                     \
    }                                                                                                               \
  } while (0)

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? (size_t)atoll(argv[1]) : 256;
  const int log2t = argc > 2 ? atoi(argv[2]) : 10;
  const size_t steps = argc > 3 ? (size_t)atoi(argv[3]) : 4;
  const int log2e = argc > 4 ? atoi(argv[4]) : (log2t >= 2 ? log2t - 2 : log2t);
  if (n < 1 || n > (1u << 20) || log2t < 1 || log2t > 16 || steps < 1 || steps > 1024 || log2e < 0 || log2e > log2t) {
    fprintf(stderr, "usage: eval_farm [chains] [log2 t] [steps] [log2 every <= log2 t]\n");
    return 2;
  }
  const uint64_t t = 1ull << log2t, every = 1ull << log2e, rounds = steps * t;
  const size_t per_step = (size_t)(t / every), per_chain = steps * per_step + 1;

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  /* ---- the farm: N chains, the states every `every` rounds ---- */
  vdf_state* initial = (vdf_state*)malloc(n * sizeof(vdf_state));
  vdf_state* cps = (vdf_state*)malloc(n * per_chain * sizeof(vdf_state));
  const size_t pairs = n * (per_chain - 1);
  vdf_state* from = (vdf_state*)malloc(pairs * sizeof(vdf_state));
  vdf_state* to = (vdf_state*)malloc(pairs * sizeof(vdf_state));
  int* ok = (int*)malloc(pairs * sizeof(int));
  if (!initial || !cps || !from || !to || !ok) return 1;
  for (size_t w = 0; w < n; ++w) {
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 1000 + w, &initial[w].x), "element");
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &initial[w].y), "element");
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 7 * w, &initial[w].i), "element");
  }
  double a = now_ms();
  CHECK(vdf_minroot_eval_batch(ctx, VDF_FIELD_FQ, initial, n, rounds, every, 0, cps), "eval_batch");
  const double eval_ms = now_ms() - a;
  printf("evaluated %zu chains x %llu rounds on the device: %.1f ms (%.2f M rounds/s), %zu checkpoints each\n", n,
         (unsigned long long)rounds, eval_ms, (double)n * (double)rounds / eval_ms * 1e-3, per_chain);

  /* ---- every interval of every chain, by the inverse walk ---- */
  for (size_t w = 0; w < n; ++w)
    for (size_t k = 0; k + 1 < per_chain; ++k) {
      from[w * (per_chain - 1) + k] = cps[w * per_chain + k];
      to[w * (per_chain - 1) + k] = cps[w * per_chain + k + 1];
    }
  a = now_ms();
  CHECK(vdf_minroot_check_batch(ctx, VDF_FIELD_FQ, to, from, pairs, every, ok), "check_batch");
  printf("checked %zu intervals of %llu rounds: %.1f ms\n", pairs, (unsigned long long)every, now_ms() - a);
  size_t bad_chains = 0;
  int* chain_ok = (int*)malloc(n * sizeof(int));
  if (!chain_ok) return 1;
  for (size_t w = 0; w < n; ++w) {
    chain_ok[w] = memcmp(&cps[w * per_chain], &initial[w], sizeof(vdf_state)) == 0;
    for (size_t k = 0; k + 1 < per_chain; ++k) chain_ok[w] = chain_ok[w] && ok[w * (per_chain - 1) + k] == 1;
    bad_chains += !chain_ok[w];
  }

  /* ---- two of them into the prover ---- */
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params_ex(ctx, t, VDF_CIRCUIT_MINROOT_FORWARD, VDF_GENS_TRY_AND_INCREMENT, &pp), "public_params");
  const size_t chosen[2] = {0, n - 1};
  int proved[2] = {0, 0}, same_as_host[2] = {0, 0};
  for (int c = 0; c < (n > 1 ? 2 : 1); ++c) {
    const size_t w = chosen[c];
    const vdf_state* mine = &cps[w * per_chain];
    vdf_fe z0[3];
    vdf_circuits* circuits = NULL;
    CHECK(vdf_nova_circuits_forward_begin(t, &initial[w], z0, &circuits), "forward_begin");
    for (size_t s = 0; s < steps; ++s) CHECK(vdf_nova_circuits_push_checkpoints(circuits, every, mine + s * per_step), "push_checkpoints");
    CHECK(vdf_nova_circuits_materialize(ctx, circuits, 0, steps, 1, NULL), "materialize");
    vdf_proof* proof = NULL;
    for (size_t k = 0; k < steps; ++k) CHECK(vdf_nova_prove_step(pp, &proof, circuits, k, z0), "prove_step");
    const vdf_state* last = mine + per_chain - 1;
    const vdf_fe zi[3] = {last->x, last->y, last->i};
    int v = 0, swapped = 1;
    CHECK(vdf_nova_verify(proof, pp, steps, z0, zi, &v), "verify");
    CHECK(vdf_nova_verify(proof, pp, steps, zi, z0, &swapped), "verify (swapped)");
    proved[c] = v && !swapped;
    vdf_state host_final;
    CHECK(vdf_minroot_eval(VDF_FIELD_FQ, VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL, &initial[w], rounds, &host_final, NULL), "eval (host)");
    same_as_host[c] = memcmp(&host_final, last, sizeof(vdf_state)) == 0;
    vdf_nova_proof_free(proof);
    vdf_nova_circuits_free(circuits);
  }

  int all_ok = bad_chains == 0;
  for (size_t w = 0; w < n; ++w) {
    int c = w == chosen[0] ? 0 : (w == chosen[1] ? 1 : -1);
    if (c >= 0) {
      printf("chain %zu: check: %s; proved %zu steps, verify: %s; final state equals the host's: %s\n", w, chain_ok[w] ? "ok" : "FAILED", steps,
             proved[c] ? "true" : "FALSE", same_as_host[c] ? "yes" : "NO");
      all_ok = all_ok && proved[c] && same_as_host[c];
    } else {
      printf("chain %zu: check: %s\n", w, chain_ok[w] ? "ok" : "FAILED");
    }
  }
  printf("%zu chains, %zu failed their check\n", n, bad_chains);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  free(chain_ok); free(ok); free(to); free(from); free(cps); free(initial);
  return all_ok ? 0 : 1;
}
