/* MANY chains of a delay function the library did not write in ONE proof, in plain C: examples/prove_custom_chain.c with the chains
 * side by side in the lanes of one step circuit.  The round is written three times as callbacks, and then
 *
 *   2 L chains evaluated on the GPU, one entry per `every` rounds kept,   vdf_round_tape_eval_batch
 *   the array left in device memory
 *   chains L .. 2 L - 1 of that array, unchanged, as the L lanes of one   vdf_nova_custom_chain_lanes_from_checkpoints
 *   chain object (lane_stride = the entries per chain)
 *   every step proved: L * (t / every) walks per step, one launch per     vdf_nova_prove_recursively_custom
 *   slice for a whole window; the circuit hands its step's trace of        (vdf_cs_repeat_lanes, vdf_cs_step_advice)
 *   L * (t + 1) entries to ONE repeat of L lanes
 *   verify, compress ONCE, verify                                         vdf_nova_verify_custom, vdf_nova_compress
 *
 * The round is (x, y) -> ((x + y)^(1/5), x + i0 + j); chain w starts at (x0 + w, 0) with the counter 1000 w.
 * Build:  cc -O2 examples/prove_custom_lanes.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/prove_custom_lanes
 * Run:    examples/prove_custom_lanes [iterations per step = 65] [rounds per checkpoint = 13] [steps = 3] [lanes = 3] [x0 = 123]
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

typedef struct { uint64_t t; size_t lanes; vdf_fe t_elem; } rounds;      /* no per-step state: the step's trace comes from vdf_cs_step_advice */

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

/* z = (x_0, y_0, i_0, x_1, y_1, i_1, ...): the lanes' carries and counters gathered lane-major, ONE repeat for all of them */
static int synthesize(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  const rounds* r = (const rounds*)self;
  const vdf_round_body body = {1, 2, 2, round_body, NULL};
  vdf_num inv[VDF_TAPE_MAX_LANES], carry[2 * VDF_TAPE_MAX_LANES], out[2 * VDF_TAPE_MAX_LANES];
  for (size_t l = 0; l < r->lanes; ++l) { carry[2 * l] = z_in[3 * l]; carry[2 * l + 1] = z_in[3 * l + 1]; inv[l] = z_in[3 * l + 2]; }
  if (vdf_cs_repeat_lanes(cs, &body, r->t, r->lanes, inv, carry, vdf_cs_is_witness(cs) ? vdf_cs_step_advice(cs) : NULL, (size_t)r->t + 1, out) != VDF_OK)
    return 1;
  const vdf_num tt = vdf_cs_const(cs, &r->t_elem);
  for (size_t l = 0; l < r->lanes; ++l) { z_out[3 * l] = out[2 * l]; z_out[3 * l + 1] = out[2 * l + 1]; z_out[3 * l + 2] = vdf_cs_add(cs, z_in[3 * l + 2], tt); }
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
  const size_t steps = argc > 3 ? (size_t)atoi(argv[3]) : 3;
  const size_t L = argc > 4 ? (size_t)atoi(argv[4]) : 3;
  const uint64_t x0 = argc > 5 ? strtoull(argv[5], NULL, 10) : 123;
  if (t < 1 || t > (1u << 20) || steps < 1 || steps > 64 || every < 1 || t % every || L < 1 || L > VDF_TAPE_MAX_LANES) {
    fprintf(stderr, "usage: prove_custom_lanes [t] [every (divides t)] [steps <= 64] [lanes <= 16] [x0]\n");
    return 2;
  }
  const size_t per_chain = steps * (size_t)(t / every) + 1;      /* checkpoints of one chain: entries of (x, y) */
  const size_t chains = 2 * L;

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  /* the field elements the example states itself, into Montgomery form: t, and per proved lane x0, its first and its last counter */
  vdf_fe plain[1 + 3 * VDF_TAPE_MAX_LANES], elem[1 + 3 * VDF_TAPE_MAX_LANES];
  memset(plain, 0, sizeof(plain));
  plain[0].l[0] = t;
  for (size_t l = 0; l < L; ++l) {
    plain[1 + 3 * l].l[0] = x0 + L + l;
    plain[2 + 3 * l].l[0] = 1000 * (L + l);
    plain[3 + 3 * l].l[0] = 1000 * (L + l) + steps * t;
  }
  CHECK(vdf_fe_to_mont(ctx, VDF_FIELD_FQ, plain, 1 + 3 * L, elem), "fe_to_mont");
  const vdf_fe zero = {{0, 0, 0, 0}};

  rounds r = {t, L, elem[0]};
  const vdf_step_circuit circuit = {3 * L, synthesize, &r};
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params_custom(ctx, &circuit, VDF_GENS_TRY_AND_INCREMENT, &pp), "public_params_custom");
  uint8_t digest[32];
  CHECK(vdf_nova_pp_digest(pp, digest), "pp_digest");
  printf("digest: ");
  for (int k = 31; k >= 0; --k) printf("%02x", digest[k]);
  printf("\n");
  uint64_t pp_lanes = 0;
  vdf_nova_pp_repeat_lanes(pp, &pp_lanes);
  printf("lanes of the repeat: %llu\n", (unsigned long long)pp_lanes);

  /* both directions of the round as tapes */
  static vdf_tape_op f_ops[VDF_TAPE_MAX_OPS], w_ops[VDF_TAPE_MAX_OPS];
  static vdf_fe f_consts[VDF_TAPE_MAX_CONSTS], w_consts[VDF_TAPE_MAX_CONSTS];
  const vdf_walk_body fb = {1, 2, forward_body, NULL}, wb = {1, 2, walk_body, NULL};
  vdf_round_tape forward, walk;
  CHECK(vdf_nova_forward_body_record(VDF_FIELD_FQ, &fb, f_ops, f_consts, &forward), "forward_body_record");
  CHECK(vdf_nova_walk_body_record(VDF_FIELD_FQ, &wb, w_ops, w_consts, &walk), "walk_body_record");

  /* 2 L chains evaluated on the device, chain w from (x0 + w, 0) under the counter 1000 w + j (inv = 0): the checkpoint array
   * stays in device memory, per_chain entries per chain */
  vdf_fe first[2 * 2 * VDF_TAPE_MAX_LANES];
  memset(plain, 0, sizeof(plain));
  for (size_t w = 0; w < chains; ++w) plain[w].l[0] = x0 + w;
  CHECK(vdf_fe_to_mont(ctx, VDF_FIELD_FQ, plain, chains, first), "fe_to_mont");
  for (size_t w = chains; w-- > 0;) { first[2 * w] = first[w]; first[2 * w + 1] = zero; }
  void* d_cps = NULL;
  CHECK(vdf_dev_alloc(ctx, chains * per_chain * 2 * sizeof(vdf_fe), &d_cps), "dev_alloc");
  CHECK(vdf_round_tape_eval_batch(ctx, VDF_FIELD_FQ, &forward, &zero, first, chains, steps * t, every, 0, 0, 1000, (vdf_fe*)d_cps), "round_tape_eval_batch");
  CHECK(vdf_ctx_sync(ctx), "ctx_sync");
  printf("evaluated: %zu chains of %llu rounds, %zu checkpoints each\n", chains, (unsigned long long)(steps * t), per_chain);

  /* chains L .. 2 L - 1 as the lanes of ONE chain object, straight from the device array: inv = 0 for every lane, and the walk
   * that produces a lane's entry 1 sees that lane's first counter */
  const vdf_fe* d_lanes = (const vdf_fe*)d_cps + L * per_chain * 2;
  vdf_fe inv[VDF_TAPE_MAX_LANES];
  uint64_t j_base[VDF_TAPE_MAX_LANES];
  for (size_t l = 0; l < L; ++l) { inv[l] = zero; j_base[l] = 1000 * (L + l); }
  vdf_custom_chain* chain = NULL;
  CHECK(vdf_nova_custom_chain_lanes_from_checkpoints(VDF_FIELD_FQ, &walk, inv, t, every, steps, L, d_lanes, per_chain, j_base, &chain),
        "custom_chain_lanes_from_checkpoints");
  vdf_fe z0[3 * VDF_TAPE_MAX_LANES], zi[3 * VDF_TAPE_MAX_LANES];
  for (size_t l = 0; l < L; ++l) {
    z0[3 * l] = elem[1 + 3 * l]; z0[3 * l + 1] = zero; z0[3 * l + 2] = elem[2 + 3 * l];
    CHECK(vdf_dev_memcpy(ctx, &zi[3 * l], d_lanes + (l * per_chain + per_chain - 1) * 2, 2 * sizeof(vdf_fe)), "dev_memcpy");
    zi[3 * l + 2] = elem[3 + 3 * l];
  }

  vdf_proof* proof = NULL;
  CHECK(vdf_nova_prove_recursively_custom(pp, &circuit, chain, z0, 2, VDF_CUSTOM_CHECK_STEPS, &proof), "prove_recursively_custom");
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
  printf("compressed proof: %zu bytes for %zu chains\ncompressed proof sha256: ", wire_len, L);
  for (int k = 0; k < 32; ++k) printf("%02x", hash[k]);
  printf("\n");

  free(wire);
  vdf_nova_snark_free(received);
  vdf_nova_snark_free(snark);
  vdf_nova_proof_free(proof);
  vdf_nova_custom_chain_free(chain);
  vdf_dev_free(ctx, d_cps);
  vdf_nova_pp_free(pp);
  vdf_ctx_destroy(ctx);
  return ok1 && ok2 ? 0 : 1;
}
