/* A delay function the library did not write, proved from its checkpoints by the CHAIN OBJECT, in plain C: the flow of
 * examples/prove_custom_pipeline.c with its hand-made window replaced by vdf_custom_chain.  The chain's round is written three
 * times as callbacks (the slow direction, the fast direction, the round to prove), and then
 *
 *   evaluation on the GPU: one entry per `every` rounds kept             vdf_round_tape_eval_batch
 *   the chain: the walk tape, inv and the checkpoints on the host        vdf_nova_custom_chain_from_checkpoints
 *   every step proved, the walks of window w + 1 on a side queue under   vdf_nova_prove_recursively_custom
 *   the proving of window w, at most two windows of traces in HBM;       (VDF_CUSTOM_CHECK_STEPS: every step's fresh instance
 *   the circuit reads its step's trace through vdf_cs_step_advice         scanned for an unsatisfied row)
 *   verify, compress, verify                                             vdf_nova_verify_custom, vdf_nova_compress
 *
 * The round is (x, y) -> ((x + y)^(1/5), x + i0 + j), so that the proof can be compared with the other examples'.
 * Build:  cc -O2 examples/prove_custom_chain.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/prove_custom_chain
 * Run:    examples/prove_custom_chain [iterations per step = 65] [rounds per checkpoint = 13] [steps = 5] [steps per window = 2] [x0 = 123]
 *         It prints the parameters' digest (a 250-bit integer, hexadecimal) and the SHA-256 of the compressed proof's bytes.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vdf_nova.h"

#define CHECK(expr, what)                                                                                         \
  do {                                                                                                              \
    int rc_ = (expr);                                                                                               \
    if (rc_ != VDF_OK) { fprintf(stderr, "%s failed (%d): %s / %s\n", what, rc_, vdf_nova_last_error(), vdf_last_error(NULL)); return 1; } \
  } while (0)

typedef struct { uint64_t t; vdf_fe t_elem; } rounds;      /* no per-step state: the step's trace comes from vdf_cs_step_advice */

/* 5^-1 mod (q - 1), q the order of Pallas (the field of the primary circuit): a plain integer, little-endian words */
static const uint64_t FIFTH_ROOT[4] = {0xd69f2280cccccccdull, 0x4e9ee0c9a143ba4aull, 0x3333333333333333ull, 0x3333333333333333ull};

/* the slow direction: entry j + 1 from entry j.  x' = (x + y)^(1/5), y' = x + i0 + j; inv[0] = i0, the chain's first counter */
static int forward_body(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* cur, vdf_num* next_out) {
  (void)self;
  next_out[0] = vdf_cs_pow(cs, vdf_cs_add(cs, cur[0], cur[1]), FIFTH_ROOT);
  next_out[1] = vdf_cs_add(cs, cur[0], vdf_cs_add(cs, inv[0], j));
  return 0;
}

/* the same round backwards: entry j from entry j + 1.  x = y' - (i0 + j), y = x'^5 - x */
static int walk_body(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* next, vdf_num* cur_out) {
  (void)self;
  const vdf_num x = vdf_cs_sub(cs, next[1], vdf_cs_add(cs, inv[0], j));
  const vdf_num x2 = vdf_cs_mul(cs, next[0], next[0]);
  const vdf_num x5 = vdf_cs_mul(cs, vdf_cs_mul(cs, x2, x2), next[0]);
  cur_out[0] = x;
  cur_out[1] = vdf_cs_sub(cs, x5, x);
  return 0;
}

/* ... and as constraints: x' is taken from the next entry of the trace and bound by x'^5 = x + y; y' = x + i_in + j */
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
  if (vdf_cs_repeat(cs, &body, r->t, &z_in[2], z_in, vdf_cs_is_witness(cs) ? vdf_cs_step_advice(cs) : NULL, z_out) != VDF_OK) return 1;
  z_out[2] = vdf_cs_add(cs, z_in[2], vdf_cs_const(cs, &r->t_elem));
  return 0;
}

/* SHA-256 (FIPS 180-4) of a byte string, to name the proof */
static uint32_t ror(uint32_t x, int n) { return x >> n | x << (32 - n); }
static void sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
      0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
      0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
      0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
      0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
      0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const size_t total = (len + 9 + 63) / 64 * 64;
  for (size_t off = 0; off < total; off += 64) {
    uint8_t blk[64];
    for (size_t k = 0; k < 64; ++k) {
      const size_t p = off + k;
      blk[k] = p < len ? msg[p] : p == len ? 0x80 : p >= total - 8 ? (uint8_t)(((uint64_t)len * 8) >> (8 * (total - 1 - p))) : 0;
    }
    uint32_t w[64], s[8];
    for (int k = 0; k < 16; ++k) w[k] = (uint32_t)blk[4 * k] << 24 | (uint32_t)blk[4 * k + 1] << 16 | (uint32_t)blk[4 * k + 2] << 8 | blk[4 * k + 3];
    for (int k = 16; k < 64; ++k)
      w[k] = w[k - 16] + (ror(w[k - 15], 7) ^ ror(w[k - 15], 18) ^ w[k - 15] >> 3) + w[k - 7] + (ror(w[k - 2], 17) ^ ror(w[k - 2], 19) ^ w[k - 2] >> 10);
    memcpy(s, h, sizeof(s));
    for (int k = 0; k < 64; ++k) {
      const uint32_t t1 = s[7] + (ror(s[4], 6) ^ ror(s[4], 11) ^ ror(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + K[k] + w[k];
      const uint32_t t2 = (ror(s[0], 2) ^ ror(s[0], 13) ^ ror(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
      s[7] = s[6]; s[6] = s[5]; s[5] = s[4]; s[4] = s[3] + t1; s[3] = s[2]; s[2] = s[1]; s[1] = s[0]; s[0] = t1 + t2;
    }
    for (int k = 0; k < 8; ++k) h[k] += s[k];
  }
  for (int k = 0; k < 32; ++k) out[k] = (uint8_t)(h[k / 4] >> (8 * (3 - k % 4)));
}

int main(int argc, char** argv) {
  const uint64_t t = argc > 1 ? strtoull(argv[1], NULL, 10) : 65;
  const uint64_t every = argc > 2 ? strtoull(argv[2], NULL, 10) : 13;
  const size_t steps = argc > 3 ? (size_t)atoi(argv[3]) : 5;
  const size_t window_steps = argc > 4 ? (size_t)atoi(argv[4]) : 2;
  const uint64_t x0 = argc > 5 ? strtoull(argv[5], NULL, 10) : 123;
  if (t < 1 || t > (1u << 20) || steps < 1 || steps > 64 || every < 1 || t % every) {
    fprintf(stderr, "usage: prove_custom_chain [t] [every (divides t)] [steps <= 64] [steps per window] [x0]\n");
    return 2;
  }
  const size_t per = (size_t)(t / every), walks = steps * per;      /* checkpoint intervals per step, and of the chain */

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  /* the few field elements the example states itself, into Montgomery form: x0, t, and the counter the chain ends on */
  const vdf_fe plain[3] = {{{x0, 0, 0, 0}}, {{t, 0, 0, 0}}, {{steps * t, 0, 0, 0}}};
  vdf_fe elem[3];
  CHECK(vdf_fe_to_mont(ctx, VDF_FIELD_FQ, plain, 3, elem), "fe_to_mont");
  const vdf_fe zero = {{0, 0, 0, 0}};

  rounds r = {t, elem[1]};
  const vdf_step_circuit circuit = {3, synthesize, &r};
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params_custom(ctx, &circuit, VDF_GENS_TRY_AND_INCREMENT, &pp), "public_params_custom");
  uint8_t digest[32];
  CHECK(vdf_nova_pp_digest(pp, digest), "pp_digest");
  printf("digest: ");
  for (int k = 31; k >= 0; --k) printf("%02x", digest[k]);
  printf("\n");

  /* both directions of the round as tapes */
  static vdf_tape_op f_ops[VDF_TAPE_MAX_OPS], w_ops[VDF_TAPE_MAX_OPS];
  static vdf_fe f_consts[VDF_TAPE_MAX_CONSTS], w_consts[VDF_TAPE_MAX_CONSTS];
  const vdf_walk_body fb = {1, 2, forward_body, NULL}, wb = {1, 2, walk_body, NULL};
  vdf_round_tape forward, walk;
  CHECK(vdf_nova_forward_body_record(VDF_FIELD_FQ, &fb, f_ops, f_consts, &forward), "forward_body_record");
  CHECK(vdf_nova_walk_body_record(VDF_FIELD_FQ, &wb, w_ops, w_consts, &walk), "walk_body_record");
  printf("forward tape: %zu ops, %u slots; walk tape: %zu ops, %u slots\n", forward.n_ops, forward.n_slots, walk.n_ops, walk.n_slots);

  /* evaluation on the device keeps one entry per `every` rounds: cps[k] = (x, y) after k * every rounds, k = 0 .. walks */
  const vdf_fe z0[3] = {elem[0], zero, zero}, first[2] = {elem[0], zero};
  vdf_fe* cps = (vdf_fe*)malloc((walks + 1) * 2 * sizeof(vdf_fe));
  if (!cps) return 1;
  CHECK(vdf_round_tape_eval_batch(ctx, VDF_FIELD_FQ, &forward, &zero, first, 1, steps * t, every, 0, 0, 0, cps), "round_tape_eval_batch");
  const vdf_fe zi[3] = {cps[2 * walks], cps[2 * walks + 1], elem[2]};

  /* the chain: inv = (i0 = 0), the walk that produces entry 1 sees j = 0.  It keeps copies: cps is the caller's again */
  vdf_custom_chain* chain = NULL;
  CHECK(vdf_nova_custom_chain_from_checkpoints(VDF_FIELD_FQ, &walk, &zero, t, every, steps, cps, 0, &chain), "custom_chain_from_checkpoints");
  uint64_t host_bytes = 0;
  CHECK(vdf_nova_custom_chain_host_bytes(chain, &host_bytes), "custom_chain_host_bytes");
  printf("chain: %zu steps, %llu bytes on the host\n", vdf_nova_custom_chain_len(chain), (unsigned long long)host_bytes);

  vdf_proof* proof = NULL;
  CHECK(vdf_nova_prove_recursively_custom(pp, &circuit, chain, z0, window_steps, VDF_CUSTOM_CHECK_STEPS, &proof), "prove_recursively_custom");
  size_t resident = 0;
  uint64_t device_bytes = 0;
  CHECK(vdf_nova_custom_chain_memory(chain, &resident, &device_bytes), "custom_chain_memory");
  printf("resident after the proof: %zu steps, %llu bytes\n", resident, (unsigned long long)device_bytes);
  int ok1 = 0, ok2 = 0;
  CHECK(vdf_nova_verify_custom(proof, pp, steps, z0, zi, &ok1), "verify_custom");
  printf("verify: %s\n", ok1 ? "true" : "FALSE");

  vdf_snark* snark = NULL;
  CHECK(vdf_nova_compress(proof, pp, &snark), "compress");
  const size_t wire_len = vdf_nova_snark_serialized_size(snark);
  uint8_t* wire = (uint8_t*)malloc(wire_len);
  vdf_snark* received = NULL;
  if (!wire) return 1;
  CHECK(vdf_nova_snark_serialize(snark, wire, wire_len), "serialize");
  CHECK(vdf_nova_snark_deserialize(pp, wire, wire_len, &received), "deserialize");
  CHECK(vdf_nova_verify_compressed(received, pp, steps, z0, zi, &ok2), "verify_compressed");
  printf("verify (compressed): %s\n", ok2 ? "true" : "FALSE");
  uint8_t hash[32];
  sha256(wire, wire_len, hash);
  printf("compressed proof: %zu bytes\ncompressed proof sha256: ", wire_len);
  for (int k = 0; k < 32; ++k) printf("%02x", hash[k]);
  printf("\n");

  free(wire);
  vdf_nova_snark_free(received);
  vdf_nova_snark_free(snark);
  vdf_nova_proof_free(proof);
  vdf_nova_custom_chain_free(chain);
  free(cps);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return ok1 && ok2 ? 0 : 1;
}
