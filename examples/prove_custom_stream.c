/* A delay function with no cheap inverse, proved WHILE IT IS EVALUATED, in plain C: the Rescue-shaped round of
 * examples/prove_rescue_chain.c (two state elements, a root layer and a power layer, round constants from a table) handed to
 * vdf_nova_eval_and_prove_custom.  Library threads evaluate the chain with the forward tape on the host; this thread is handed every
 * finished step as checkpoints, has the step's trace rebuilt on the GPU by the SAME forward tape, proves it and lets it go.  The
 * proof exists one step after the chain's last round, whatever the chain's length -- and there is no inverse tape in this file.
 *
 *   the round as a forward tape                                           vdf_nova_forward_body_record
 *   evaluate, hand over, rebuild, prove, release: one call                vdf_nova_eval_and_prove_custom
 *   verify, compress, verify                                              vdf_nova_verify_custom, vdf_nova_compress
 *
 * `every` = 0 hands whole traces over instead of checkpoints (nothing is rebuilt on the device).  `rows` must divide t.
 * Build:  cc -O2 examples/prove_custom_stream.c -Iinclude -Lvdf_amd -lvdf_nova -lvdf_hip -Wl,-rpath,'$ORIGIN/../vdf_amd' -o examples/prove_custom_stream
 * Run:    examples/prove_custom_stream [iterations per step = 64] [rounds per checkpoint = 8] [steps = 4] [rows = 8] [s0 = 123]
 *         It prints the parameters' digest, the stream's figures, the SHA-256 of the running proof's wire bytes, the verdicts and the
 *         SHA-256 of the compressed proof.
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

typedef struct {
  uint64_t t;
  const vdf_fe* table;      /* rows x 2, Montgomery form, host memory: the one table of both bodies */
  size_t rows;
  vdf_fe two, three;        /* the entries of M, Montgomery form */
  vdf_pow_step chain[VDF_POW_CHAIN_MAX_STEPS];
  size_t n_steps;
} rounds;

/* everything behind the root layer, in either kind of body: (s0', s1') = M (M (r0, r1) + c)^5 */
static void after_the_roots(const rounds* r, vdf_cs* cs, vdf_num r0, vdf_num r1, vdf_num out[2]) {
  const vdf_num a[2] = {vdf_cs_add(cs, vdf_cs_add(cs, vdf_cs_scale(cs, r0, &r->two), r1), vdf_cs_tab(cs, r->table, r->rows, 2, 0)),
                        vdf_cs_add(cs, vdf_cs_add(cs, r0, vdf_cs_scale(cs, r1, &r->three)), vdf_cs_tab(cs, r->table, r->rows, 2, 1))};
  vdf_num p[2];
  for (int i = 0; i < 2; ++i) {
    const vdf_num q = vdf_cs_mul(cs, a[i], a[i]);
    p[i] = vdf_cs_mul(cs, vdf_cs_mul(cs, q, q), a[i]);
  }
  out[0] = vdf_cs_add(cs, vdf_cs_scale(cs, p[0], &r->two), p[1]);
  out[1] = vdf_cs_add(cs, p[0], vdf_cs_scale(cs, p[1], &r->three));
}

static int forward_body(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* cur, vdf_num* next_out) {
  const rounds* r = (const rounds*)self;
  (void)j; (void)inv;
  next_out[2] = vdf_cs_pow_chain(cs, cur[0], r->chain, r->n_steps);
  next_out[3] = vdf_cs_pow_chain(cs, cur[1], r->chain, r->n_steps);
  after_the_roots(r, cs, next_out[2], next_out[3], next_out);
  return 0;
}

static int round_body(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* carry, const vdf_num* cur, const vdf_num* next,
                      vdf_num* carry_out) {
  const rounds* r = (const rounds*)self;
  (void)j; (void)inv; (void)cur;
  vdf_num root[2];
  for (int i = 0; i < 2; ++i) {
    root[i] = vdf_cs_alloc_from(cs, next[2 + i]);
    const vdf_num t1 = vdf_cs_mul(cs, root[i], root[i]);
    if (vdf_cs_enforce(cs, vdf_cs_mul(cs, t1, t1), root[i], carry[i]) != VDF_OK) return 1;
  }
  after_the_roots(r, cs, root[0], root[1], carry_out);
  return 0;
}

static int synthesize(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out) {
  const rounds* r = (const rounds*)self;
  const vdf_round_body body = {0, 2, 4, round_body, self};
  return vdf_cs_repeat(cs, &body, r->t, NULL, z_in, vdf_cs_is_witness(cs) ? vdf_cs_step_advice(cs) : NULL, z_out) != VDF_OK;
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

static void print_sha256(const char* what, const uint8_t* bytes, size_t len) {
  uint8_t hash[32];
  sha256(bytes, len, hash);
  printf("%s: %zu bytes\n%s sha256: ", what, len, what);
  for (int k = 0; k < 32; ++k) printf("%02x", hash[k]);
  printf("\n");
}

int main(int argc, char** argv) {
  const uint64_t t = argc > 1 ? strtoull(argv[1], NULL, 10) : 64;
  const uint64_t every = argc > 2 ? strtoull(argv[2], NULL, 10) : 8;
  const size_t steps = argc > 3 ? (size_t)atoi(argv[3]) : 4;
  const size_t rows = argc > 4 ? (size_t)atoi(argv[4]) : 8;
  const uint64_t s0 = argc > 5 ? strtoull(argv[5], NULL, 10) : 123;
  if (t < 1 || t > (1u << 20) || steps < 1 || steps > 64 || (every && t % every) || rows < 1 || rows > VDF_TAPE_MAX_TAB_ROWS || t % rows) {
    fprintf(stderr, "usage: prove_custom_stream [t] [every (divides t; 0: whole traces)] [steps <= 64] [rows (divides t)] [s0]\n");
    return 2;
  }

  int device = 0;
  vdf_ctx* ctx = NULL;
  if (vdf_ctx_create(&device, 1, &ctx) != VDF_OK) { fprintf(stderr, "no GPU: %s\n", vdf_last_error(NULL)); return 1; }

  /* the table: row r = (c0, c1) = (1000 + 7 r, 1 + r^2); then s0, 2 and 3, into Montgomery form */
  vdf_fe* plain = (vdf_fe*)calloc(2 * rows + 3, sizeof(vdf_fe));
  vdf_fe* table = (vdf_fe*)calloc(2 * rows + 3, sizeof(vdf_fe));
  if (!plain || !table) return 1;
  for (size_t r = 0; r < rows; ++r) { plain[2 * r].l[0] = 1000 + 7 * r; plain[2 * r + 1].l[0] = 1 + r * r; }
  plain[2 * rows].l[0] = s0; plain[2 * rows + 1].l[0] = 2; plain[2 * rows + 2].l[0] = 3;
  CHECK(vdf_fe_to_mont(ctx, VDF_FIELD_FQ, plain, 2 * rows + 3, table), "fe_to_mont");
  const vdf_fe s0_elem = table[2 * rows], zero = {{0, 0, 0, 0}};

  static rounds r;
  r.t = t; r.table = table; r.rows = rows; r.two = table[2 * rows + 1]; r.three = table[2 * rows + 2];
  CHECK(vdf_minroot_pow_chain(VDF_FIELD_FQ, r.chain, VDF_POW_CHAIN_MAX_STEPS, &r.n_steps), "minroot_pow_chain");
  const vdf_step_circuit circuit = {2, synthesize, &r};
  vdf_pp* pp = NULL;
  CHECK(vdf_nova_public_params_custom(ctx, &circuit, VDF_GENS_TRY_AND_INCREMENT, &pp), "public_params_custom");
  uint8_t digest[32];
  CHECK(vdf_nova_pp_digest(pp, digest), "pp_digest");
  printf("digest: ");
  for (int k = 31; k >= 0; --k) printf("%02x", digest[k]);
  printf("\n");

  /* the one direction the round has, as a tape: it names the table by the caller's pointer (host memory), which is what both the
   * evaluator's threads and the chain (which makes its own device copy) read */
  static vdf_tape_op f_ops[VDF_TAPE_MAX_OPS];
  static vdf_fe f_consts[VDF_TAPE_MAX_CONSTS];
  const vdf_walk_body fb = {0, 4, forward_body, &r};
  vdf_round_tape forward;
  CHECK(vdf_nova_forward_body_record(VDF_FIELD_FQ, &fb, f_ops, f_consts, &forward), "forward_body_record");
  printf("forward tape: %zu ops, %u slots, table %u x %u\n", forward.n_ops, forward.n_slots, forward.tab_rows, forward.tab_cols);

  const vdf_fe entry0[4] = {s0_elem, zero, zero, zero};      /* the state, and no roots: nothing produced entry 0 */
  const vdf_fe z0[3] = {s0_elem, zero, zero};                /* (arity 2: the third element is room the declarations of z0[3] ask for) */
  const uint64_t j_base = 0;
  vdf_nova_custom_stream stream;
  memset(&stream, 0, sizeof(stream));
  stream.forward_tape = &forward;                            /* no inv, no walk tape: the steps are rebuilt by the forward tape */
  stream.t = t; stream.every = every; stream.lanes = 1; stream.j_base = &j_base;
  vdf_fe last[4];
  vdf_proof* proof = NULL;
  vdf_nova_stream_stats stats;
  CHECK(vdf_nova_eval_and_prove_custom(pp, &circuit, &stream, entry0, steps, z0, last, &proof, &stats), "eval_and_prove_custom");
  printf("stream: %llu steps, evaluation %.3f ms, proof %.3f ms behind the output, backlog at most %llu\n", (unsigned long long)stats.steps,
         stats.eval_ms, stats.after_eval_ms, (unsigned long long)stats.max_backlog);
  const vdf_fe zi[3] = {last[0], last[1], zero};

  const size_t run_len = vdf_nova_proof_serialized_size(proof);
  uint8_t* run = (uint8_t*)malloc(run_len);
  if (!run) return 1;
  CHECK(vdf_nova_proof_serialize(proof, run, run_len), "proof_serialize");
  print_sha256("running proof", run, run_len);

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
  print_sha256("compressed proof", wire, wire_len);

  free(wire);
  free(run);
  vdf_nova_snark_free(received);
  vdf_nova_snark_free(snark);
  vdf_nova_proof_free(proof);
  vdf_nova_pp_free(pp);
  free(table);
  free(plain);
  vdf_ctx_destroy(ctx);
  return ok1 && ok2 ? 0 : 1;
}
