/* A prover beside an evaluator, in plain C: the chain is evaluated FIRST and only its checkpoints are kept -- what a
 * fast sequential evaluator (another process, another machine) hands over -- and the prover works from those alone.
 *
 *   the evaluator: forward MinRoot rounds, one state kept every `every` rounds   vdf_minroot_eval_checkpoints
 *   the prover:    circuits from the states, no trace anywhere                   vdf_nova_circuits_from_checkpoints
 *                  traces rebuilt on the GPU by inverse walks, window by window,
 *                  under the proving of the window before                        vdf_nova_prove_recursively_windowed
 *   verification of the recursive proof                                          vdf_nova_verify
 *
 * Reads nothing from disk.  A wrong checkpoint cannot go unnoticed: every walk must land on the checkpoint before it.
 * Build:  cc -O2 examples/prove_from_checkpoints.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/prove_from_checkpoints
 * Run:    examples/prove_from_checkpoints [log2 iterations per step = 10] [steps = 6] [log2 every = log2 t] [window steps = 2]
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
    if (rc_ != VDF_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc_, vdf_nova_last_error()); return 1; }   \
  } while (0)

int main(int argc, char** argv) {
  const int log2t = argc > 1 ? atoi(argv[1]) : 10;
  const size_t steps = argc > 2 ? (size_t)atoi(argv[2]) : 6;
  const int log2e = argc > 3 ? atoi(argv[3]) : log2t;
  const size_t window = argc > 4 ? (size_t)atoi(argv[4]) : 2;
  if (log2t < 1 || log2t > 20 || steps < 1 || steps > 100000 || log2e < 0 || log2e > log2t) {
    fprintf(stderr, "usage: prove_from_checkpoints [log2 t] [steps] [log2 every <= log2 t] [window steps]\n");
    return 2;
  }
  const uint64_t t = 1ull << log2t, every = 1ull << log2e;

  /* ---- the evaluator's side: states only ---- */
  vdf_state initial;
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, 123, &initial.x), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &initial.y), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &initial.i), "element");
  const size_t n_states = steps * (size_t)(t / every) + 1;
  vdf_state* states = (vdf_state*)malloc(n_states * sizeof(vdf_state));
  if (!states) return 1;
  double a = now_ms();
  CHECK(vdf_minroot_eval_checkpoints(VDF_FIELD_FQ, VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL, &initial, steps * t, every, states), "eval_checkpoints");
  printf("forward evaluation of %zu x 2^%d rounds (host): %.0f ms, %zu checkpoints = %zu bytes handed over\n", steps, log2t,
         now_ms() - a, n_states, n_states * sizeof(vdf_state));

  /* ---- the prover's side ---- */
  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params(ctx, t, &pp), "public_params");
  vdf_fe z0[3];
  vdf_circuits* circuits = NULL;
  CHECK(vdf_nova_circuits_from_checkpoints(t, every, steps, states, z0, &circuits), "circuits_from_checkpoints");
  free(states);                                    /* everything else is forgotten: the circuits hold the checkpoints */

  a = now_ms();
  vdf_proof* proof = NULL;
  CHECK(vdf_nova_prove_recursively_windowed(pp, circuits, t, z0, window, &proof), "prove_recursively_windowed");
  printf("prove_recursively over checkpoints, %zu steps in windows of %zu: %.2f ms\n", steps, window, now_ms() - a);
  size_t resident = 0;
  uint64_t bytes = 0;
  CHECK(vdf_nova_circuits_memory(circuits, &resident, &bytes), "circuits_memory");
  printf("traces left on the device: %zu steps, %llu bytes\n", resident, (unsigned long long)bytes);

  const vdf_fe zi[3] = {initial.x, initial.y, initial.i};
  int ok = 0;
  CHECK(vdf_nova_verify(proof, pp, steps, z0, zi, &ok), "verify");
  printf("verify: %s\n", ok ? "true" : "FALSE");

  vdf_nova_proof_free(proof);
  vdf_nova_circuits_free(circuits);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return ok && resident == 0 ? 0 : 1;
}
