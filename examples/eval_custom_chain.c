/* Many chains of a delay function of the caller's own evaluated on the GPU, its power taken by the caller's own ADDITION CHAIN,
 * in plain C: no Python, no torch, no HIP headers.
 *
 *   the forward round, written once as a callback: next = ((x + y)^(1/5), x + j)          vdf_nova_forward_body_record
 *   its fifth root by an addition chain instead of square-and-multiply (283 products,     vdf_cs_pow_chain
 *     not 377, and all of them in the lazy domain on the device)
 *   the chain itself: here the library's own for MinRoot, so that there is something      vdf_minroot_pow_chain
 *     to compare with; a chain for any other exponent comes from                          vdf_nova_pow_chain_window
 *   N chains evaluated at once, one lane each                                             vdf_round_tape_eval_batch
 *   the same chains by the built-in evaluator, and the comparison                         vdf_minroot_eval_batch
 *
 * A THROUGHPUT arrangement, not a faster VDF: one chain on a lane is far slower than on a host core.
 * Build:  cc -O2 examples/eval_custom_chain.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/eval_custom_chain
 * Run:    examples/eval_custom_chain [chains = 130] [rounds = 64]
 *         exit status 0 iff every chain ends where vdf_minroot_eval_batch ends.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vdf_nova.h"

#define CHECK(expr, what)                                                                                         \
  do {                                                                                                              \
    int rc_ = (expr);                                                                                               \
    if (rc_ != VDF_OK) {                                                                                            \
      fprintf(stderr, "%s failed (%d): %s | %s\n", what, rc_, vdf_nova_last_error(), vdf_last_error(ctx));         \
      return 1;                                                                                                     \
    }                                                                                                               \
  } while (0)

typedef struct { vdf_pow_step steps[VDF_POW_CHAIN_MAX_STEPS]; size_t n_steps; } root_chain;

/* entry j = (x, y) -> entry j + 1 = ((x + y)^(1/5), x + j) */
static int forward_round(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* cur, vdf_num* next_out) {
  const root_chain* rc = (const root_chain*)self;
  (void)inv;
  next_out[0] = vdf_cs_pow_chain(cs, vdf_cs_add(cs, cur[0], cur[1]), rc->steps, rc->n_steps);
  next_out[1] = vdf_cs_add(cs, cur[0], j);
  return 0;
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? (size_t)atoll(argv[1]) : 130;
  const uint64_t rounds = argc > 2 ? (uint64_t)atoll(argv[2]) : 64;
  if (n < 1 || n > (1u << 20) || rounds < 1 || rounds > (1u << 20)) {
    fprintf(stderr, "usage: eval_custom_chain [chains] [rounds]\n");
    return 2;
  }
  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  /* ---- the chain and what it computes ---- */
  root_chain rc;
  CHECK(vdf_minroot_pow_chain(VDF_FIELD_FQ, rc.steps, VDF_POW_CHAIN_MAX_STEPS, &rc.n_steps), "minroot_pow_chain");
  uint64_t e[4], products = 0;
  uint32_t n_tmp = 0;
  CHECK(vdf_nova_pow_chain_exponent(rc.steps, rc.n_steps, e, &n_tmp, &products), "pow_chain_exponent");
  printf("chain: %zu steps, %u temporaries, %llu products, exponent %016llx%016llx%016llx%016llx\n", rc.n_steps, n_tmp,
         (unsigned long long)products, (unsigned long long)e[3], (unsigned long long)e[2], (unsigned long long)e[1], (unsigned long long)e[0]);

  /* ---- the round, recorded ---- */
  vdf_tape_op ops[VDF_TAPE_MAX_OPS];
  vdf_fe consts[VDF_TAPE_MAX_CONSTS];
  vdf_round_tape tape;
  const vdf_walk_body body = {0, 2, forward_round, &rc};
  CHECK(vdf_nova_forward_body_record(VDF_FIELD_FQ, &body, ops, consts, &tape), "forward_body_record");
  printf("tape: %zu ops, %zu constants, %u slots\n", tape.n_ops, tape.n_consts, tape.n_slots);

  /* ---- N chains through the tape and through the built-in evaluator ---- */
  vdf_state* initial = (vdf_state*)malloc(n * sizeof(vdf_state));
  vdf_state* want = (vdf_state*)malloc(n * sizeof(vdf_state));
  vdf_fe* start = (vdf_fe*)malloc(n * 2 * sizeof(vdf_fe));
  vdf_fe* got = (vdf_fe*)malloc(n * 2 * sizeof(vdf_fe));
  if (!initial || !want || !start || !got) return 1;
  for (size_t w = 0; w < n; ++w) {
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 1000 + w, &initial[w].x), "element");
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, w, &initial[w].y), "element");
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 7 * w, &initial[w].i), "element");
    start[2 * w] = initial[w].x;
    start[2 * w + 1] = initial[w].y;
  }
  /* chain w's counter starts at 7 w: VDF_TAPE_J = j_base + w * j_walk_step + the rounds behind it */
  CHECK(vdf_round_tape_eval_batch(ctx, VDF_FIELD_FQ, &tape, NULL, start, n, rounds, 0, 0, 0, 7, got), "round_tape_eval_batch");
  CHECK(vdf_minroot_eval_batch(ctx, VDF_FIELD_FQ, initial, n, rounds, 0, 0, want), "minroot_eval_batch");
  size_t differ = 0;
  for (size_t w = 0; w < n; ++w)
    differ += memcmp(&got[2 * w], &want[w].x, sizeof(vdf_fe)) != 0 || memcmp(&got[2 * w + 1], &want[w].y, sizeof(vdf_fe)) != 0;
  uint64_t fnv = 0xcbf29ce484222325ull;
  const uint8_t* bytes = (const uint8_t*)got;
  for (size_t k = 0; k < n * 2 * sizeof(vdf_fe); ++k) { fnv ^= bytes[k]; fnv *= 0x100000001b3ull; }
  printf("chains: %zu x %llu rounds\ndiffer from vdf_minroot_eval_batch: %zu\nfinal entries fnv1a64: %016llx\n", n,
         (unsigned long long)rounds, differ, (unsigned long long)fnv);
  vdf_ctx_destroy(ctx);
  free(got); free(start); free(want); free(initial);
  return differ == 0 ? 0 : 1;
}
