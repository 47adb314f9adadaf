/* A verifier that never holds a prover's object: compressed proofs come in as files of wire bytes ("VDFSNK03", what
 * examples/prove_chain writes with its fifth argument) and go straight to vdf_nova_verify_wire_batch -- the points of every
 * proof are decoded on the GPU (vdf_points_decompress), the proofs verified as one batch.  Plain C, the two C ABIs only.
 *
 * Build:  cc -O2 examples/verify_wire.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/verify_wire
 * Run:    examples/verify_wire <log2 iterations per step> <steps> <x0> <i0> <file> [<file> ...]
 *         the statement is prove_chain's: the chain of steps x 2^k rounds from (x0, 0, i0).  Its end, the output the prover
 *         claims, is recomputed here by evaluating the chain on the host (a verifier in the field is handed it); every file is
 *         checked against that one statement.  One line per file: "entry <k>: ok=<0|1> status=<code> <file>", then "all_ok=<0|1>".
 *         A file that does not decode (status != 0) or does not verify is a verdict, not a failure: the exit status is 0
 *         whenever the batch call ran.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vdf_nova.h"

#define CHECK(expr, what)                                                                                         \
  do {                                                                                                              \
    int rc_ = (expr);                                                                                               \
    if (rc_ != VDF_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc_, vdf_nova_last_error()); return 1; }   \
  } while (0)

#define MAX_FILES 64

int main(int argc, char** argv) {
  if (argc < 6 || argc - 5 > MAX_FILES) { fprintf(stderr, "usage: verify_wire <log2 t> <steps> <x0> <i0> <file> [<file> ...]\n"); return 2; }
  const int log2t = atoi(argv[1]);
  const size_t steps = (size_t)atoi(argv[2]);
  if (log2t < 1 || log2t > 20 || steps < 1 || steps > 1000) { fprintf(stderr, "log2 t in 1..20, steps in 1..1000\n"); return 2; }
  const uint64_t t = 1ull << log2t;
  const size_t count = (size_t)(argc - 5);

  static uint8_t* blob[MAX_FILES];
  static size_t len[MAX_FILES], num_steps[MAX_FILES];
  for (size_t k = 0; k < count; ++k) {
    FILE* f = fopen(argv[5 + k], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[5 + k]); return 2; }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    blob[k] = (uint8_t*)malloc(size > 0 ? (size_t)size : 1);
    len[k] = size > 0 ? fread(blob[k], 1, (size_t)size, f) : 0;
    fclose(f);
    num_steps[k] = steps;
  }

  vdf_state initial, end;
  if (strlen(argv[3]) == 64) {                      /* x0 as prove_chain takes it: a small integer, or the 32 bytes of a vdf_fe in hex */
    uint8_t raw[32];
    for (int k = 0; k < 32; ++k) {
      unsigned byte = 0;
      if (sscanf(argv[3] + 2 * k, "%2x", &byte) != 1) { fprintf(stderr, "x0: not hex\n"); return 2; }
      raw[k] = (uint8_t)byte;
    }
    memcpy(&initial.x, raw, 32);
  } else {
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, strtoull(argv[3], NULL, 10), &initial.x), "element");
  }
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &initial.y), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FQ, strtoull(argv[4], NULL, 10), &initial.i), "element");
  CHECK(vdf_minroot_eval(VDF_FIELD_FQ, VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL, &initial, t * steps, &end, NULL), "minroot_eval");
  /* the inverse step circuit runs from the chain's end back to its start: z0 is the end, zi the start */
  vdf_fe* z0 = (vdf_fe*)malloc(count * 3 * sizeof(vdf_fe));
  vdf_fe* zi = (vdf_fe*)malloc(count * 3 * sizeof(vdf_fe));
  for (size_t k = 0; k < count; ++k) {
    z0[3 * k] = end.x; z0[3 * k + 1] = end.y; z0[3 * k + 2] = end.i;
    zi[3 * k] = initial.x; zi[3 * k + 1] = initial.y; zi[3 * k + 2] = initial.i;
  }

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params(ctx, t, &pp), "public_params");

  static int ok[MAX_FILES], status[MAX_FILES];
  int all_ok = 0;
  CHECK(vdf_nova_verify_wire_batch(pp, count, (const uint8_t* const*)blob, len, num_steps, z0, zi, ok, status, &all_ok), "verify_wire_batch");
  for (size_t k = 0; k < count; ++k) printf("entry %zu: ok=%d status=%d %s\n", k, ok[k], status[k], argv[5 + k]);
  printf("all_ok=%d\n", all_ok);

  for (size_t k = 0; k < count; ++k) free(blob[k]);
  free(z0); free(zi);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return 0;
}
