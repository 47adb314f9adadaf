/* Several MinRoot chains evaluated on the GPU and proved by ONE Nova proof, in plain C: no Python, no torch, no HIP headers.
 *
 *   L chains evaluated at once, a state kept every `every` rounds                     vdf_minroot_eval_batch
 *   parameters of the forward circuit in L lanes (arity 3L)                           vdf_nova_public_params_lanes
 *   a chain of steps that advance all L lanes by t rounds                             vdf_nova_circuits_lanes_begin
 *     one step from every lane's t / every + 1 states, straight out of the batch      vdf_nova_circuits_push_checkpoints_lanes
 *   traces rebuilt by inverse walks, one fold per step                                vdf_nova_prove_recursively
 *   z0 = the L initial states, zi = the L final states                                vdf_nova_verify
 *   one compressed proof for all L chains                                             vdf_nova_compress, vdf_nova_verify_compressed
 *   the L outputs against the L inputs by the inverse walk (the reference's check)    vdf_minroot_check_batch
 *
 * Build:  cc -O2 examples/prove_lanes.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/prove_lanes
 * Run:    examples/prove_lanes [lanes = 3] [log2 iterations per step = 6] [steps = 2] [x of lane 0 = 1000] [output file]
 *         Lane l starts at (x + l, 0, 7 l).  Exit status 0 iff both verifications pass, the tampered ones fail and every
 *         output checks; the compressed proof's wire bytes ("VDFSNK03") go to the output file when one is named.
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

int main(int argc, char** argv) {
  const size_t lanes = argc > 1 ? (size_t)atoll(argv[1]) : 3;
  const int log2t = argc > 2 ? atoi(argv[2]) : 6;
  const size_t steps = argc > 3 ? (size_t)atoi(argv[3]) : 2;
  const uint64_t x0 = argc > 4 ? (uint64_t)atoll(argv[4]) : 1000;
  const char* out_path = argc > 5 ? argv[5] : NULL;
  if (lanes < 1 || lanes > VDF_NOVA_MAX_LANES || log2t < 0 || log2t > 16 || steps < 1 || steps > 1024) {
    fprintf(stderr, "usage: prove_lanes [lanes <= %d] [log2 t <= 16] [steps] [x] [output file]\n", VDF_NOVA_MAX_LANES);
    return 2;
  }
  const uint64_t t = 1ull << log2t, every = log2t >= 2 ? t / 4 : t, rounds = steps * t;
  const size_t per_step = (size_t)(t / every), per_chain = steps * per_step + 1;

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  /* ---- the L chains on the device: lane l's states every `every` rounds at cps[l * per_chain + k] ---- */
  vdf_state* initial = (vdf_state*)malloc(lanes * sizeof(vdf_state));
  vdf_state* cps = (vdf_state*)malloc(lanes * per_chain * sizeof(vdf_state));
  vdf_state* final = (vdf_state*)malloc(lanes * sizeof(vdf_state));
  vdf_fe* z0 = (vdf_fe*)malloc(3 * lanes * sizeof(vdf_fe));
  vdf_fe* zi = (vdf_fe*)malloc(3 * lanes * sizeof(vdf_fe));
  int* ok = (int*)malloc(lanes * sizeof(int));
  if (!initial || !cps || !final || !z0 || !zi || !ok) return 1;
  for (size_t l = 0; l < lanes; ++l) {
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, x0 + l, &initial[l].x), "element");
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &initial[l].y), "element");
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 7 * l, &initial[l].i), "element");
  }
  CHECK(vdf_minroot_eval_batch(ctx, VDF_FIELD_FQ, initial, lanes, rounds, every, 0, cps), "eval_batch");
  printf("evaluated %zu chains x %llu rounds on the device, %zu checkpoints each\n", lanes, (unsigned long long)rounds, per_chain);

  /* ---- one proof for all of them ---- */
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params_lanes(ctx, t, lanes, VDF_GENS_TRY_AND_INCREMENT, NULL, NULL, &pp), "public_params_lanes");
  uint64_t nc = 0, nv = 0, eb = 0, en = 0;
  CHECK(vdf_nova_pp_sizes(pp, VDF_SIDE_PRIMARY, &nc, &nv, NULL, NULL, NULL), "pp_sizes");
  CHECK(vdf_nova_pp_early_rows(pp, &eb, &en), "pp_early_rows");
  printf("lanes %zu, primary shape %llu x %llu, %llu early rows, stencil code %d\n", vdf_nova_pp_lanes(pp), (unsigned long long)nc,
         (unsigned long long)nv, (unsigned long long)en, vdf_nova_pp_stencil(pp));
  vdf_circuits* circuits = NULL;
  CHECK(vdf_nova_circuits_lanes_begin(t, lanes, initial, z0, &circuits), "lanes_begin");
  for (size_t s = 0; s < steps; ++s)
    CHECK(vdf_nova_circuits_push_checkpoints_lanes(circuits, every, cps + s * per_step, per_chain), "push_checkpoints_lanes");
  vdf_proof* proof = NULL;
  CHECK(vdf_nova_prove_recursively(pp, circuits, t, z0, &proof), "prove_recursively");
  for (size_t l = 0; l < lanes; ++l) {
    final[l] = cps[l * per_chain + per_chain - 1];
    zi[3 * l] = final[l].x; zi[3 * l + 1] = final[l].y; zi[3 * l + 2] = final[l].i;
  }
  int v = 0, v_bad = 1, vc = 0, vc_bad = 1;
  CHECK(vdf_nova_verify(proof, pp, steps, z0, zi, &v), "verify");
  printf("verify: %s\n", v ? "true" : "false");
  if (lanes > 1) {                                  /* the outputs of lanes 0 and 1 swapped: another statement */
    vdf_fe tmp[3];
    memcpy(tmp, zi, sizeof(tmp)); memcpy(zi, zi + 3, sizeof(tmp)); memcpy(zi + 3, tmp, sizeof(tmp));
    CHECK(vdf_nova_verify(proof, pp, steps, z0, zi, &v_bad), "verify (swapped)");
    memcpy(tmp, zi, sizeof(tmp)); memcpy(zi, zi + 3, sizeof(tmp)); memcpy(zi + 3, tmp, sizeof(tmp));
  } else {
    CHECK(vdf_nova_verify(proof, pp, steps, zi, z0, &v_bad), "verify (swapped)");
  }
  printf("verify with two outputs swapped: %s\n", v_bad ? "true" : "false");
  vdf_snark* snark = NULL;
  CHECK(vdf_nova_compress(proof, pp, &snark), "compress");
  CHECK(vdf_nova_verify_compressed(snark, pp, steps, z0, zi, &vc), "verify_compressed");
  printf("verify (compressed): %s\n", vc ? "true" : "false");
  CHECK(vdf_nova_verify_compressed(snark, pp, steps + 1, z0, zi, &vc_bad), "verify_compressed (one step more)");
  const size_t wire_len = vdf_nova_snark_serialized_size(snark);
  uint8_t* wire = (uint8_t*)malloc(wire_len);
  if (!wire) return 1;
  CHECK(vdf_nova_snark_serialize(snark, wire, wire_len), "snark_serialize");
  printf("one compressed proof for %zu chains: %zu bytes on the wire\n", lanes, wire_len);
  if (out_path) {
    FILE* f = fopen(out_path, "wb");
    if (!f || fwrite(wire, 1, wire_len, f) != wire_len) { fprintf(stderr, "cannot write %s\n", out_path); return 1; }
    fclose(f);
  }

  /* ---- the L outputs against the L inputs ---- */
  CHECK(vdf_minroot_check_batch(ctx, VDF_FIELD_FQ, final, initial, lanes, rounds, ok), "check_batch");
  int all_ok = v && !v_bad && vc && !vc_bad;
  for (size_t l = 0; l < lanes; ++l) {
    printf("lane %zu: check: %s\n", l, ok[l] == 1 ? "ok" : "FAILED");
    all_ok = all_ok && ok[l] == 1;
  }
  vdf_nova_snark_free(snark);
  vdf_nova_proof_free(proof);
  vdf_nova_circuits_free(circuits);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  free(wire); free(ok); free(zi); free(z0); free(final); free(cps); free(initial);
  return all_ok ? 0 : 1;
}
