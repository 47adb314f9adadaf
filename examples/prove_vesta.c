/* Prove a VestaVDF chain (MinRoot over Fp) in plain C: the curve cycle in the OTHER orientation, G1 = Vesta, G2 = Pallas.
 *
 *   parameters of the forward step circuit over Fp                        vdf_nova_public_params_field(VDF_FIELD_FP, ...)
 *   evaluation on a library thread (it runs the parameters' field)        vdf_nova_eval_and_prove
 *   verification of the running proof: z0 = initial state, zi = final     vdf_nova_verify
 *   compression, verification, the wire, verification of the decoded one  vdf_nova_compress / vdf_nova_verify_compressed / _serialize
 *
 * A proof attests a chain over ONE field; the secondary circuit (over Fq here) is still TrivialTestCircuit.
 * Build:  cc -O2 examples/prove_vesta.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/prove_vesta
 * Run:    examples/prove_vesta [log2 iterations per step = 6] [steps = 3] [x0 = 123] [i0 = 0]
 *         It prints the parameters' digest and the SHA-256 of the "VDFSNK03" bytes so that a caller can compare them with
 *         another host's for the same chain.
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

/* SHA-256 (FIPS 180-4), for the one digest this client prints */
static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static void sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
      0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
      0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
      0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
      0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
      0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const size_t total = ((len + 9 + 63) / 64) * 64;
  for (size_t off = 0; off < total; off += 64) {
    uint8_t blk[64];
    for (size_t k = 0; k < 64; ++k) {
      const size_t p = off + k;
      blk[k] = p < len ? msg[p] : p == len ? 0x80 : p >= total - 8 ? (uint8_t)(((uint64_t)len * 8) >> (8 * (total - 1 - p))) : 0;
    }
    uint32_t w[64];
    for (int k = 0; k < 16; ++k) w[k] = (uint32_t)blk[4 * k] << 24 | (uint32_t)blk[4 * k + 1] << 16 | (uint32_t)blk[4 * k + 2] << 8 | blk[4 * k + 3];
    for (int k = 16; k < 64; ++k)
      w[k] = w[k - 16] + (ror(w[k - 15], 7) ^ ror(w[k - 15], 18) ^ (w[k - 15] >> 3)) + w[k - 7] + (ror(w[k - 2], 17) ^ ror(w[k - 2], 19) ^ (w[k - 2] >> 10));
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int k = 0; k < 64; ++k) {
      const uint32_t t1 = hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + K[k] + w[k];
      const uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  for (int k = 0; k < 8; ++k) { out[4 * k] = (uint8_t)(h[k] >> 24); out[4 * k + 1] = (uint8_t)(h[k] >> 16); out[4 * k + 2] = (uint8_t)(h[k] >> 8); out[4 * k + 3] = (uint8_t)h[k]; }
}

static void print_hex(const char* label, const uint8_t* p, size_t n) {
  printf("%s: ", label);
  for (size_t k = 0; k < n; ++k) printf("%02x", p[k]);
  printf("\n");
}

int main(int argc, char** argv) {
  const int log2t = argc > 1 ? atoi(argv[1]) : 6;
  const size_t steps = argc > 2 ? (size_t)atoi(argv[2]) : 3;
  if (log2t < 1 || log2t > 20 || steps < 1 || steps > 100000) { fprintf(stderr, "usage: prove_vesta [log2 t] [steps] [x0] [i0]\n"); return 2; }
  const uint64_t t = 1ull << log2t;
  const uint64_t x0 = argc > 3 ? strtoull(argv[3], NULL, 10) : 123;
  const uint64_t i0 = argc > 4 ? strtoull(argv[4], NULL, 10) : 0;

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  vdf_state initial, final_state, expect;
  CHECK(vdf_minroot_element(VDF_FIELD_FP, x0, &initial.x), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FP, 0, &initial.y), "element");
  CHECK(vdf_minroot_element(VDF_FIELD_FP, i0, &initial.i), "element");

  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params_field(ctx, VDF_FIELD_FP, t, VDF_CIRCUIT_MINROOT_FORWARD, 1, VDF_GENS_TRY_AND_INCREMENT, NULL, NULL, &pp),
        "public_params_field");
  uint8_t digest[32];
  CHECK(vdf_nova_pp_digest(pp, digest), "pp_digest");
  printf("public_params(2^%d, forward, Fp): orientation %s, stencil code %d\n", log2t, vdf_nova_pp_field(pp) == VDF_FIELD_FP ? "Fp" : "Fq",
         vdf_nova_pp_stencil(pp));
  print_hex("digest", digest, 32);

  vdf_proof* proof = NULL;
  CHECK(vdf_nova_eval_and_prove(pp, VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL, &initial, steps, &final_state, &proof, NULL), "eval_and_prove");
  CHECK(vdf_minroot_eval(VDF_FIELD_FP, VDF_MODE_LTR_SEQUENTIAL, &initial, t * steps, &expect, NULL), "eval");
  int all_ok = memcmp(&expect, &final_state, sizeof(expect)) == 0;
  printf("final state is VestaVDF's: %s\n", all_ok ? "true" : "FALSE");
  print_hex("final state", (const uint8_t*)&final_state, sizeof(final_state));

  const vdf_fe z0[3] = {initial.x, initial.y, initial.i};
  const vdf_fe zi[3] = {final_state.x, final_state.y, final_state.i};
  int ok = 0;
  CHECK(vdf_nova_verify(proof, pp, steps, z0, zi, &ok), "verify");
  printf("verify: %s\n", ok ? "true" : "FALSE");
  all_ok = all_ok && ok;
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
  uint8_t md[32];
  vdf_snark* received = NULL;
  CHECK(vdf_nova_snark_serialize(snark, wire, wire_len), "serialize");
  sha256(wire, wire_len, md);
  printf("wire bytes: %zu\n", wire_len);
  print_hex("wire sha256", md, 32);
  CHECK(vdf_nova_snark_deserialize(pp, wire, wire_len, &received), "deserialize");
  CHECK(vdf_nova_verify_compressed(received, pp, steps, z0, zi, &ok), "verify_compressed (decoded)");
  printf("verify (decoded): %s\n", ok ? "true" : "FALSE");
  all_ok = all_ok && ok;

  free(wire);
  vdf_nova_snark_free(received);
  vdf_nova_snark_free(snark);
  vdf_nova_proof_free(proof);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return all_ok ? 0 : 1;
}
