/* A verifier of an aggregate that holds bytes only: a file of "VDFAGG01" wire bytes (what examples/aggregate_proofs writes, or
 * AggregateProof.serialize) and a text file of the statements go straight to vdf_nova_verify_aggregate_wire -- every point of the
 * encoding is decoded on the GPU (vdf_points_decompress), the per-entry folds and both accumulators are made there
 * (vdf_points_axpy, vdf_msm_batch), the hashes and the exact checks run on the host -- or, with the optional fourth argument, the
 * three Poseidon hashes of every entry on the GPU as well (vdf_ro_hash_batch).  Plain C, the two C ABIs only.
 *
 * Build:  cc -O2 examples/verify_aggregate.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/verify_aggregate
 * Run:    examples/verify_aggregate <iterations per step> <aggregate file> <statements file> [<ro device min count>]
 *         the optional last argument is vdf_nova_pp_set_verify_ro_device's: from that many entries on the per-entry hashes are
 *         made on the GPU (0, or no argument: on the host); the line that comes out does not depend on it.
 *         the parameter set is the default one (the reference's inverse MinRoot step circuit, arity 3) at that many iterations
 *         per step.  The statements file has one line per entry, in the aggregate's order:
 *             <num_steps> <z0[0]> <z0[1]> <z0[2]> <zi[0]> <zi[1]> <zi[2]>
 *         each element the 32 bytes of a vdf_fe (Montgomery form, as the C ABI passes it) in 64 hex digits.
 *         One line comes out: "count=<K> ok=<0|1> bad_entry=<k|-1> decode_code=<code>".  Bytes that do not decode or do not
 *         verify are a verdict, not a failure: the exit status is 0 whenever the call ran.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vdf_nova.h"

#define CHECK(expr, what)                                                                                         \
  do {                                                                                                              \
    int rc_ = (expr);                                                                                               \
    if (rc_ != VDF_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc_, vdf_nova_last_error()); return 1; }   \
  } while (0)

static int hex_fe(const char* s, vdf_fe* out) {
  uint8_t raw[32];
  if (strlen(s) != 64) return 0;
  for (int k = 0; k < 32; ++k) {
    unsigned byte = 0;
    if (sscanf(s + 2 * k, "%2x", &byte) != 1) return 0;
    raw[k] = (uint8_t)byte;
  }
  memcpy(out, raw, 32);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5) {
    fprintf(stderr, "usage: verify_aggregate <iterations per step> <aggregate file> <statements file> [<ro device min count>]\n");
    return 2;
  }
  const uint64_t t = strtoull(argv[1], NULL, 10);
  if (t < 1 || t > (1ull << 20)) { fprintf(stderr, "iterations per step in 1..2^20\n"); return 2; }

  FILE* f = fopen(argv[2], "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* blob = (uint8_t*)malloc(size > 0 ? (size_t)size : 1);
  const size_t len = size > 0 ? fread(blob, 1, (size_t)size, f) : 0;
  fclose(f);

  static size_t num_steps[VDF_NOVA_AGGREGATE_MAX];
  vdf_fe* z0 = (vdf_fe*)malloc(VDF_NOVA_AGGREGATE_MAX * 3 * sizeof(vdf_fe));
  vdf_fe* zi = (vdf_fe*)malloc(VDF_NOVA_AGGREGATE_MAX * 3 * sizeof(vdf_fe));
  size_t count = 0;
  f = fopen(argv[3], "r");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
  for (;;) {
    unsigned long long steps;
    char e[6][80];
    const int got = fscanf(f, "%llu %79s %79s %79s %79s %79s %79s", &steps, e[0], e[1], e[2], e[3], e[4], e[5]);
    if (got == EOF) break;
    if (got != 7 || count == VDF_NOVA_AGGREGATE_MAX) { fprintf(stderr, "statements: line %zu is malformed, or there are too many\n", count + 1); return 2; }
    num_steps[count] = (size_t)steps;
    for (int k = 0; k < 3; ++k)
      if (!hex_fe(e[k], &z0[3 * count + k]) || !hex_fe(e[3 + k], &zi[3 * count + k])) { fprintf(stderr, "statements: line %zu: not 64 hex digits\n", count + 1); return 2; }
    ++count;
  }
  fclose(f);

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params(ctx, t, &pp), "public_params");
  if (argc == 5) CHECK(vdf_nova_pp_set_verify_ro_device(pp, atoi(argv[4])), "pp_set_verify_ro_device");

  int ok = 0, decode_code = 0;
  int64_t bad_entry = -1;
  CHECK(vdf_nova_verify_aggregate_wire(pp, blob, len, count, num_steps, z0, zi, &ok, &bad_entry, &decode_code), "verify_aggregate_wire");
  printf("count=%zu ok=%d bad_entry=%" PRId64 " decode_code=%d\n", count, ok, bad_entry, decode_code);

  free(blob); free(z0); free(zi);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return 0;
}
