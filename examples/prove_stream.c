/* Prove a MinRoot chain WHILE it is evaluated, in plain C: no Python, no torch, no HIP headers.
 *
 *   parameters of the forward step circuit                                vdf_nova_public_params_ex(VDF_CIRCUIT_MINROOT_FORWARD)
 *   evaluation on a library thread, one prove_step per finished step      vdf_nova_eval_and_prove
 *   verification of the running proof: z0 = initial state, zi = final     vdf_nova_verify
 *   compression, verification, the wire                                    vdf_nova_compress / vdf_nova_verify_compressed / _serialize
 *
 * The proof is complete one step after the evaluator's last round, whatever the chain's length (after_eval_ms below).
 * Build:  cc -O2 examples/prove_stream.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/prove_stream
 * Run:    examples/prove_stream [log2 iterations per step = 10] [steps = 8] [x0 = 123] [i0 = 0] [file]
 *         file: where the compressed proof's wire bytes go.  It prints the final state (the 96 bytes of a vdf_state in hex) so
 *         that a caller can compare it with vdf_minroot_eval's (tests/test_gpu_forward.py does).
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
  const size_t steps = argc > 2 ? (size_t)atoi(argv[2]) : 8;
  if (log2t < 1 || log2t > 20 || steps < 1 || steps > 100000) { fprintf(stderr, "usage: prove_stream [log2 t] [steps] [x0] [i0] [file]\n"); return 2; }
  const uint64_t t = 1ull << log2t;
  const uint64_t x0 = argc > 3 ? strtoull(argv[3], NULL, 10) : 123;
  const uint64_t i0 = argc > 4 ? strtoull(argv[4], NULL, 10) : 0;
  const char* wire_path = argc > 5 ? argv[5] : NULL;

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  vdf_state initial, final_state;
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, x0, &initial.x), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &initial.y), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, i0, &initial.i), "element");

  double a = now_ms();
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params_ex(ctx, t, VDF_CIRCUIT_MINROOT_FORWARD, VDF_GENS_TRY_AND_INCREMENT, &pp), "public_params");
  printf("public_params(2^%d, forward): %.0f ms, stencil code %d\n", log2t, now_ms() - a, vdf_nova_pp_stencil(pp));

  vdf_proof* proof = NULL;
  vdf_nova_stream_stats st;
  CHECK(vdf_nova_eval_and_prove(pp, VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL, &initial, steps, &final_state, &proof, &st), "eval_and_prove");
  printf("evaluated %zu x 2^%d rounds in %.1f ms; proof complete %.2f ms after the last round (largest backlog: %llu steps)\n", steps, log2t,
         st.eval_ms, st.after_eval_ms, (unsigned long long)st.max_backlog);
  printf("final state: ");
  for (size_t k = 0; k < sizeof(final_state); ++k) printf("%02x", ((const uint8_t*)&final_state)[k]);
  printf("\n");

  const vdf_fe z0[3] = {initial.x, initial.y, initial.i};
  const vdf_fe zi[3] = {final_state.x, final_state.y, final_state.i};
  int ok = 0;
  CHECK(vdf_nova_verify(proof, pp, steps, z0, zi, &ok), "verify");
  printf("verify: %s\n", ok ? "true" : "FALSE");
  int all_ok = ok;
  CHECK(vdf_nova_verify(proof, pp, steps, zi, z0, &ok), "verify (swapped)");
  printf("verify with z0 and zi swapped: %s\n", ok ? "TRUE" : "false");
  all_ok = all_ok && !ok;

  vdf_snark* snark = NULL;
  CHECK(vdf_nova_compress(proof, pp, &snark), "compress");
  CHECK(vdf_nova_verify_compressed(snark, pp, steps, z0, zi, &ok), "verify_compressed");
  printf("verify (compressed): %s\n", ok ? "true" : "FALSE");
  all_ok = all_ok && ok;

  const size_t wire_len = vdf_nova_snark_serialized_size(snark);
  uint8_t* wire = (uint8_t*)malloc(wire_len);
  vdf_snark* received = NULL;
  CHECK(vdf_nova_snark_serialize(snark, wire, wire_len), "serialize");
  CHECK(vdf_nova_snark_deserialize(pp, wire, wire_len, &received), "deserialize");
  CHECK(vdf_nova_verify_compressed(received, pp, steps, z0, zi, &ok), "verify_compressed (decoded)");
  printf("compressed proof on the wire: %zu bytes; decoded and verified: %s\n", wire_len, ok ? "true" : "FALSE");
  all_ok = all_ok && ok;
  if (wire_path) {
    FILE* f = fopen(wire_path, "wb");
    if (!f || fwrite(wire, 1, wire_len, f) != wire_len) { fprintf(stderr, "cannot write %s\n", wire_path); return 1; }
    fclose(f);
  }
  free(wire);
  vdf_nova_snark_free(received);
  vdf_nova_snark_free(snark);
  vdf_nova_proof_free(proof);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return all_ok ? 0 : 1;
}
