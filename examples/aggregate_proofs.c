/* Three chains of different lengths, proved apart under one parameter set, become ONE compressed proof
 * (vdf_nova_compress_aggregate, "vdf-aggregate-v1" in include/vdf_nova.h): the running instances are folded into one per side and
 * one argument per side is made.  The aggregate is written as bytes ("VDFAGG01") and verified from the bytes through a SECOND
 * parameter handle made from the same arguments -- what a verifier elsewhere would hold.  Plain C, the two C ABIs only.
 *
 * Build:  cc -O2 examples/aggregate_proofs.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/aggregate_proofs
 * Run:    examples/aggregate_proofs [log2 iterations per step] [file]
 *         chains of 1, 2 and 3 steps from x0 = 101, 102, 103; prints the sizes, the verdict and the SHA-256 of the aggregate,
 *         writes the bytes to [file] when one is given.  Exit status 0 iff the aggregate verified.
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

/* SHA-256 (FIPS 180-4), for the one line that names the aggregate */
static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static void sha256(const uint8_t* data, size_t len, uint8_t out[32]) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
      0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
      0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
      0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
      0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
      0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const size_t padded = (len + 9 + 63) / 64 * 64;
  uint8_t* m = (uint8_t*)calloc(padded, 1);
  memcpy(m, data, len);
  m[len] = 0x80;
  for (int k = 0; k < 8; ++k) m[padded - 1 - k] = (uint8_t)(((uint64_t)len * 8) >> (8 * k));
  for (size_t off = 0; off < padded; off += 64) {
    uint32_t w[64], s[8];
    for (int i = 0; i < 16; ++i)
      w[i] = (uint32_t)m[off + 4 * i] << 24 | (uint32_t)m[off + 4 * i + 1] << 16 | (uint32_t)m[off + 4 * i + 2] << 8 | m[off + 4 * i + 3];
    for (int i = 16; i < 64; ++i)
      w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    memcpy(s, h, sizeof s);
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = s[7] + (rotr(s[4], 6) ^ rotr(s[4], 11) ^ rotr(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + K[i] + w[i];
      const uint32_t t2 = (rotr(s[0], 2) ^ rotr(s[0], 13) ^ rotr(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
      s[7] = s[6]; s[6] = s[5]; s[5] = s[4]; s[4] = s[3] + t1; s[3] = s[2]; s[2] = s[1]; s[1] = s[0]; s[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i) h[i] += s[i];
  }
  free(m);
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 4; ++k) out[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
}

#define CHAINS 3

int main(int argc, char** argv) {
  const int log2t = argc > 1 ? atoi(argv[1]) : 6;
  const char* path = argc > 2 ? argv[2] : NULL;
  if (log2t < 1 || log2t > 20) { fprintf(stderr, "usage: aggregate_proofs [log2 t in 1..20] [file]\n"); return 2; }
  const uint64_t t = 1ull << log2t;

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params(ctx, t, &pp), "public_params");

  /* three provers' worth of work: chain k has k + 1 steps of t rounds from (101 + k, 0, 0) */
  vdf_proof* proofs[CHAINS] = {NULL, NULL, NULL};
  vdf_circuits* circuits[CHAINS] = {NULL, NULL, NULL};
  size_t num_steps[CHAINS];
  vdf_fe z0[CHAINS * 3], zi[CHAINS * 3];
  for (int k = 0; k < CHAINS; ++k) {
    vdf_state initial;
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 101 + (uint64_t)k, &initial.x), "element");
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &initial.y), "element");
    CHECK(vdf_minroot_element(VDF_FIELD_FQ, 0, &initial.i), "element");
    num_steps[k] = (size_t)k + 1;
    CHECK(vdf_nova_eval_and_make_circuits(VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL, t, num_steps[k], &initial, &z0[3 * k], &circuits[k]), "eval_and_make_circuits");
    CHECK(vdf_nova_circuits_upload(ctx, circuits[k]), "circuits_upload");
    CHECK(vdf_nova_prove_recursively(pp, circuits[k], t, &z0[3 * k], &proofs[k]), "prove_recursively");
    zi[3 * k] = initial.x; zi[3 * k + 1] = initial.y; zi[3 * k + 2] = initial.i;
  }

  vdf_aggregate* agg = NULL;
  CHECK(vdf_nova_compress_aggregate(pp, CHAINS, (const vdf_proof* const*)proofs, &agg), "compress_aggregate");
  const size_t len = vdf_nova_aggregate_serialized_size(agg);
  uint8_t* bytes = (uint8_t*)malloc(len);
  CHECK(vdf_nova_aggregate_serialize(agg, bytes, len), "aggregate_serialize");
  printf("aggregate of %zu proofs (1, 2 and 3 steps of 2^%d rounds): %zu bytes\n", vdf_nova_aggregate_count(agg), log2t, len);
  if (path) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(bytes, 1, len, f) != len) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    fclose(f);
  }

  /* the verifier: its own parameter handle, the bytes, the three statements */
  vdf_pp* pp_verifier = NULL;
  CHECK(vdf_nova_public_params(ctx, t, &pp_verifier), "public_params (verifier)");
  vdf_aggregate* received = NULL;
  CHECK(vdf_nova_aggregate_deserialize(pp_verifier, bytes, len, &received), "aggregate_deserialize");
  int ok = 0;
  int64_t bad_entry = -1;
  CHECK(vdf_nova_verify_aggregate(received, pp_verifier, CHAINS, num_steps, z0, zi, &ok, &bad_entry), "verify_aggregate");
  printf("verified from the bytes: %s (bad_entry = %lld)\n", ok ? "true" : "FALSE", (long long)bad_entry);
  uint8_t md[32];
  sha256(bytes, len, md);
  printf("sha256: ");
  for (int k = 0; k < 32; ++k) printf("%02x", md[k]);
  printf("\n");

  free(bytes);
  vdf_nova_aggregate_free(received);
  vdf_nova_aggregate_free(agg);
  for (int k = 0; k < CHAINS; ++k) { vdf_nova_proof_free(proofs[k]); vdf_nova_circuits_free(circuits[k]); }
  vdf_nova_pp_free(pp_verifier);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return ok ? 0 : 1;
}
