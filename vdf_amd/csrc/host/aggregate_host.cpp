// libvdf_nova.so, part 4: many running proofs under one parameter set aggregated into ONE compressed proof by folding.
//
// Protocol "vdf-aggregate-v1" (restated by tests/aggregate_spec.py).  Per proof k the prelude of vdf_nova_compress: R1_k = the
// running primary instance, F2_k = the running secondary instance folded with the last secondary one (cross-term commitment
// T2_k, the Poseidon challenge the circuits recompute).  Per side (0: the R1_k, 1: the F2_k) a transcript "aggregate" absorbs
// count | side and then EVERY instance before the first challenge is drawn; acc = instance 1, and for k = 2..K
//   TT_k = A z1 o B z2 + A z2 o B z1 - u1 C z2 - u2 C z1   (index 1: acc, index 2: instance k; vdf_cross_term_relaxed)
//   absorb commit(TT_k), r = a 128-bit challenge
//   W <- W1 + r W2, E <- E1 + r TT_k + r^2 E2, u <- u1 + r u2, X <- X1 + r X2                      (vdf_fold_relaxed, vdf_axpy)
//   comm_W <- comm_W1 + r comm_W2, comm_E <- comm_E1 + r comm_TT_k + r^2 comm_E2
// and one argument per side (compress_host.cpp, unchanged, on its own transcript "compress") for the two accumulators.
//
// Soundness: knowledge soundness of Nova's folding scheme for two relaxed instances (Kothapalli, Setty, Tzialla: "Nova",
// CRYPTO 2022, construction 1 with both instances relaxed), applied K - 1 times per side with 128-bit Fiat-Shamir challenges
// that bind every statement of the aggregate; a valid aggregate attests all K statements.  Nothing about zero knowledge is claimed.
#include "nova_internal.hpp"

using namespace vdfnova;

struct vdf_aggregate {
  struct Statement {                 // what "VDFSNK03" carries of a proof in front of its arguments
    Inst r_U1, r_U2, l_u2;
    Aff T2;
    std::vector<Fe> zi1;
    Fe zi2;
  };
  std::vector<Statement> st;
  std::vector<Aff> TT[2];            // the count - 1 cross-term commitments of each side's folds
  Spartan sp[2];                     // the arguments for the two accumulators
  uint64_t t = 0;
  uint8_t digest[32];
  int field = VDF_FIELD_FQ;          // the orientation: the primary side's scalar field
  size_t arity = 0;
};

namespace {

// a <- a + r b with the cross-term commitment TT (r: Montgomery form, raw: the same 128-bit integer): the points by host arithmetic
void fold_pair(const Side& sd, Inst& a, const Inst& b, const Aff& TT, const Fe& r, const uint64_t raw[4]) {
  const Field& F = *sd.F;
  const Field& Fb = *sd.Fb;
  const Fe r2 = from_mont(sqr(r, F), F);                                    // r^2 mod the group order, a plain 255-bit integer
  const Pt w = pt_add(pt_from_aff(a.comm_W, Fb), pt_mul(pt_from_aff(b.comm_W, Fb), raw, 128, Fb), Fb);
  Pt e = pt_add(pt_from_aff(a.comm_E, Fb), pt_mul(pt_from_aff(TT, Fb), raw, 128, Fb), Fb);
  e = pt_add(e, pt_mul(pt_from_aff(b.comm_E, Fb), r2.l, 255, Fb), Fb);
  a.comm_W = pt_to_aff(w, Fb);
  a.comm_E = pt_to_aff(e, Fb);
  a.u = add(a.u, mul(r, b.u, F), F);
  for (int j = 0; j < NUM_IO; ++j) a.X[j] = add(a.X[j], mul(r, b.X[j], F), F);
}

// Steps 2-3 of the protocol on instances alone: the transcript, the challenges (Montgomery form of the side's scalar field) and
// the folded instance.  sd: F, Fb and digest are read, nothing else.
void fold_instances_core(const Side& sd, int side, size_t count, const Inst* inst, const Aff* TT, Inst* acc, Fe* r_out) {
  const Field& F = *sd.F;
  const Field& Fb = *sd.Fb;
  Transcript tr("aggregate");
  const uint64_t head[2] = {(uint64_t)count, (uint64_t)side};
  tr.absorb("count", head, 16);
  for (size_t k = 0; k < count; ++k) instance_bytes(tr, sd, inst[k].comm_W, inst[k].comm_E, inst[k].u, inst[k].X);
  Inst a = inst[0];
  for (size_t k = 1; k < count; ++k) {
    tr.absorb_pt("T", &TT[k - 1], 1, Fb);
    uint64_t raw[4];
    const Fe r = tr.challenge("r", F, raw);
    fold_pair(sd, a, inst[k], TT[k - 1], r, raw);
    if (r_out) r_out[k - 1] = r;
  }
  *acc = a;
}

Side host_side(int field_of_primary, int side, const uint8_t digest[32]) {
  Side sd;
  sd.side = side;
  sd.field = cycle_field(field_of_primary, side);
  sd.F = &field(sd.field);
  sd.Fb = &field(cycle_field(field_of_primary, 1 - side));
  memcpy(sd.digest, digest, 32);
  return sd;
}

// one side's argument on the wire (as vdf_nova_snark_serialize lays it out: 32-byte points)
uint8_t* put_argument(uint8_t* o, const Spartan& sp, const Field& F, const Field& Fb) {
  for (const auto& ev : sp.outer) for (const Fe& v : ev) o = wire_put_fe(o, v, F);
  for (const Fe& v : sp.claims) o = wire_put_fe(o, v, F);
  for (const auto& ev : sp.inner) for (const Fe& v : ev) o = wire_put_fe(o, v, F);
  o = wire_put_fe(o, sp.w_eval, F);
  for (const Ipa* ip : {&sp.ipaW, &sp.ipaE}) {
    for (size_t j = 0; j < ip->L.size(); ++j) { pt_compress(ip->L[j], Fb, o); pt_compress(ip->R[j], Fb, o + 32); o += 64; }
    for (const Fe& v : ip->a) o = wire_put_fe(o, v, F);
  }
  return o;
}
// point(enc, sd, dst): what becomes of a 32-byte point encoding (nova_internal.hpp get_inst_points has the rule)
template <class PointFn>
const uint8_t* get_argument(const uint8_t* i, Spartan& p, const Layout& L, const Side& sd, bool* canonical, PointFn&& point) {
  const Field& F = *sd.F;
  spartan_resize(p, L);
  auto get = [&](Fe& v) { *canonical &= wire_get_fe(i, F, &v); i += 32; };
  for (auto& ev : p.outer) for (Fe& v : ev) get(v);
  for (Fe& v : p.claims) get(v);
  for (auto& ev : p.inner) for (Fe& v : ev) get(v);
  get(p.w_eval);
  for (Ipa* ip : {&p.ipaW, &p.ipaE}) {
    for (size_t j = 0; j < ip->L.size(); ++j) {
      point(i, sd, &ip->L[j]);
      point(i + 32, sd, &ip->R[j]);
      i += 64;
    }
    for (Fe& v : ip->a) get(v);
  }
  return i;
}

constexpr size_t AGG_HEADER = 8 + 8 + 8 + 32;
size_t aggregate_wire_size(size_t count, size_t arity, const Layout L[2]) {
  return AGG_HEADER + count * statement_wire(arity) + 2 * (count - 1) * 32 + spartan_wire_size(L[0]) + spartan_wire_size(L[1]);
}

// ---- "VDFAGG01" read back: the one walk over the layout (include/vdf_nova.h) ---------------------------------------------------
// What stands in front of the elements: length, magic, t, digest, count.  The codes are vdf_nova_aggregate_deserialize's.
int aggregate_wire_header(const vdf_pp* pp, const uint8_t* in, size_t len, Layout L[2], size_t* count_out) {
  if (len < AGG_HEADER) return fail(VDF_ERR_BAD_LENGTH, "encoding is shorter than its header");
  if (memcmp(in, WIRE_MAGIC_AGGREGATE, 8) != 0) return fail(VDF_ERR_BAD_ARG, "not this kind of encoding (magic)");
  uint64_t t, count;
  memcpy(&t, in + 8, 8);
  memcpy(&count, in + 16, 8);
  if (t != pp->t || memcmp(in + 24, pp->digest, 32) != 0) return fail(VDF_ERR_BAD_ARG, "encoding was made under other public parameters");
  L[0] = layout_of(pp->s[0]); L[1] = layout_of(pp->s[1]);
  if (count == 0 || count > VDF_NOVA_AGGREGATE_MAX || len != aggregate_wire_size((size_t)count, pp->arity, L))
    return fail(VDF_ERR_BAD_LENGTH, "encoding has the wrong length for this count and shape");
  *count_out = (size_t)count;
  return VDF_OK;
}
// Every element behind a header that passed: field elements are range-checked and converted here (*canonical), every point's 32
// bytes go to point(enc, side, dst) -- decoded on the spot by the host deserialiser, noted by the wire verifier for one launch per curve.
template <class PointFn>
std::unique_ptr<vdf_aggregate> aggregate_wire_walk(vdf_pp* pp, const Layout L[2], const uint8_t* in, size_t count, bool* canonical, PointFn&& point) {
  std::unique_ptr<vdf_aggregate> a(new vdf_aggregate());
  a->t = pp->t;
  a->field = pp->field;
  a->arity = pp->arity;
  memcpy(a->digest, pp->digest, 32);
  a->st.resize(count);
  const uint8_t* i = in + AGG_HEADER;
  for (vdf_aggregate::Statement& s : a->st) {
    i = get_inst_points(i, &s.r_U1, pp->s[0], true, canonical, point);
    i = get_inst_points(i, &s.r_U2, pp->s[1], true, canonical, point);
    i = get_inst_points(i, &s.l_u2, pp->s[1], false, canonical, point);
    point(i, pp->s[1], &s.T2); i += 32;
    s.zi1.resize(pp->arity);
    for (size_t k = 0; k < pp->arity; ++k, i += 32) *canonical &= wire_get_fe(i, *pp->s[0].F, &s.zi1[k]);
    *canonical &= wire_get_fe(i, *pp->s[1].F, &s.zi2); i += 32;
  }
  for (int side = 0; side < 2; ++side) {
    a->TT[side].resize(count - 1);
    for (Aff& p : a->TT[side]) { point(i, pp->s[side], &p); i += 32; }
  }
  for (int side = 0; side < 2; ++side) i = get_argument(i, a->sp[side], L[side], pp->s[side], canonical, point);
  return a;
}

// One side's accumulator on the device: z = [W | u | X], E, and A z, B z, C z kept current by the fold (they are linear in z);
// beside it the products of the incoming instance and the cross term.
struct SideFold {
  const Side& sd;
  vdf_ctx* ctx;
  void *z = nullptr, *E = nullptr, *abc[3] = {}, *abc2[3] = {}, *T = nullptr;
  Inst inst;
  size_t have = 0;
  Transcript tr{"aggregate"};
  SideFold(const Side& s, vdf_ctx* c) : sd(s), ctx(c) {}
  int alloc(DevBufs& bufs, bool folds) {
    { int rc = bufs.zeros(sd.ncols, &z); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    { int rc = bufs.zeros(sd.num_cons, &E); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    if (!folds) return VDF_OK;                       // a single proof: the accumulator is a copy of its instance
    for (void** p : {&abc[0], &abc[1], &abc[2], &abc2[0], &abc2[1], &abc2[2], &T}) {
      int rc = bufs.zeros(sd.num_cons, p);
      if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx));
    }
    return VDF_OK;
  }
  void start(size_t count, const Inst* all) {        // every instance is absorbed before the first challenge
    const uint64_t head[2] = {(uint64_t)count, (uint64_t)sd.side};
    tr.absorb("count", head, 16);
    for (size_t k = 0; k < count; ++k) instance_bytes(tr, sd, all[k].comm_W, all[k].comm_E, all[k].u, all[k].X);
  }
  // the next instance with its witness on the device (left as it is); *TT: the commitment to the cross term of a fold
  int take(const Inst& in, const void* d_z, const void* d_E, bool folds, Aff* TT) {
    const Field& F = *sd.F;
    const Field& Fb = *sd.Fb;
    if (have++ == 0) {
      inst = in;
      HIPCALL(ctx, vdf_dev_memcpy(ctx, z, d_z, sd.ncols * 32));
      HIPCALL(ctx, vdf_dev_memcpy(ctx, E, d_E, sd.num_cons * 32));
      if (folds) HIPCALL(ctx, vdf_spmv3(ctx, sd.shape, (const vdf_fe*)z, (vdf_fe*)abc[0], (vdf_fe*)abc[1], (vdf_fe*)abc[2]));
      return VDF_OK;
    }
    const size_t n = sd.num_cons;
    HIPCALL(ctx, vdf_spmv3(ctx, sd.shape, (const vdf_fe*)d_z, (vdf_fe*)abc2[0], (vdf_fe*)abc2[1], (vdf_fe*)abc2[2]));
    HIPCALL(ctx, vdf_cross_term_relaxed(ctx, sd.field, (const vdf_fe*)abc[0], (const vdf_fe*)abc[1], (const vdf_fe*)abc[2], (const vdf_fe*)&inst.u,
                                        (const vdf_fe*)abc2[0], (const vdf_fe*)abc2[1], (const vdf_fe*)abc2[2], (const vdf_fe*)&in.u, n, (vdf_fe*)T));
    vdf_jac jt;
    HIPCALL(ctx, vdf_msm(ctx, sd.gens, 0, (const vdf_fe*)T, n, 1, &jt));          // (a host result: the call waits for it)
    *TT = jac_to_aff(jt, Fb);
    tr.absorb_pt("T", TT, 1, Fb);
    uint64_t raw[4];
    const Fe r = tr.challenge("r", F, raw);
    HIPCALL(ctx, vdf_fold_relaxed(ctx, sd.field, (const vdf_fe*)&r, n, (vdf_fe*)abc[0], (vdf_fe*)abc[1], (vdf_fe*)abc[2], (vdf_fe*)E,
                                  (const vdf_fe*)abc2[0], (const vdf_fe*)abc2[1], (const vdf_fe*)abc2[2], (const vdf_fe*)d_E, (const vdf_fe*)T));
    HIPCALL(ctx, vdf_axpy(ctx, sd.field, (const vdf_fe*)z, (const vdf_fe*)&r, (const vdf_fe*)d_z, sd.ncols, (vdf_fe*)z));
    fold_pair(sd, inst, in, *TT, r, raw);                                    // the instance, as the verifier folds it
    return VDF_OK;
  }
};

// the context's asynchronous flag set for a scope and put back, with a wait, on every way out
struct AsyncScope {
  vdf_ctx* c;
  int was = 0;
  bool armed = false;
  explicit AsyncScope(vdf_ctx* ctx) : c(ctx) {}
  int enter() {
    HIPCALL(c, vdf_ctx_get_async(c, &was));
    HIPCALL(c, vdf_ctx_sync(c));
    HIPCALL(c, vdf_ctx_set_async(c, 1));
    armed = true;
    return VDF_OK;
  }
  ~AsyncScope() { if (armed) { vdf_ctx_sync(c); vdf_ctx_set_async(c, was); } }
};

// The exact checks of every entry (as vdf_nova_verify_compressed makes them) and the Poseidon challenge of the verifier's own
// secondary fold: passed(k, statement, r) receives each entry that holds, in order.  Returns the first entry that fails, -1 when none
// does.  Both verifiers (host folds, device folds) run this and nothing else per entry.
template <class Passed>
int64_t exact_checks(const vdf_aggregate* agg, const vdf_pp* pp, size_t count, const size_t num_steps[], const vdf_fe* z0, const vdf_fe* zi,
                     Passed&& passed) {
  const Side& S1 = pp->s[PRIMARY];
  const Side& S2 = pp->s[SECONDARY];
  const Field& F1 = *S1.F;
  const Field& F2 = *S2.F;
  const size_t ar = pp->arity;
  for (size_t k = 0; k < count; ++k) {
    const vdf_aggregate::Statement& s = agg->st[k];
    if (s.zi1.size() != ar) return (int64_t)k;
    const Fe* z0k = (const Fe*)z0 + k * ar;
    const std::vector<Fe> z0p(z0k, z0k + ar), z0s(1, zero()), zi2(1, s.zi2);
    uint64_t hv[4];
    hash_state(S1.field, pp->params[PRIMARY], from_u64(num_steps[k], F1), z0p, s.zi1, to_relaxed(s.r_U2, F2), hv, pp->ro);
    if (int_to_fe(hv, F2) != s.l_u2.X[0]) return (int64_t)k;
    hash_state(S2.field, pp->params[SECONDARY], from_u64(num_steps[k], F2), z0s, zi2, to_relaxed(s.r_U1, F1), hv, pp->ro);
    if (int_to_fe(hv, F2) != s.l_u2.X[1]) return (int64_t)k;
    if (memcmp(s.zi1.data(), (const Fe*)zi + k * ar, 32 * ar) != 0 || !s.zi2.is_zero()) return (int64_t)k;
    uint64_t r[4];
    fold_challenge(pp, s.r_U2, s.l_u2, s.T2, r);
    passed(k, s, r);
  }
  return -1;
}

// The device copy of what the set's oracle reads for a field, made on first use and freed with the set: the default block's 88
// round constants (vdf_nova_ro_constants' order; *mds stays null), or another block's round constants and matrix
// (vdf_nova_ro_block_constants' layout).
int ro_constants_on_device(vdf_pp* pp, int field_id, const void** rc_out, const void** mds_out) {
  std::lock_guard<std::mutex> lock(pp->ro_mu);
  auto upload = [&](void*& d, const void* src, size_t bytes) -> int {
    if (d) return VDF_OK;
    void* p = nullptr;
    HIPCALL(pp->ctx, vdf_dev_alloc(pp->ctx, bytes, &p));
    const int rc = vdf_dev_memcpy(pp->ctx, p, src, bytes);
    if (rc != VDF_OK) { vdf_dev_free(pp->ctx, p); return fail(rc, std::string("vdf_dev_memcpy (round constants): ") + vdf_last_error(pp->ctx)); }
    d = p;
    return VDF_OK;
  };
  *mds_out = nullptr;
  if (pp->ro->is_default) {
    { int rc = upload(pp->d_ro_rc[field_id], ro_constants(field_id).ext, VDF_RO_CONSTANTS * sizeof(Fe)); if (rc != VDF_OK) return rc; }
    *rc_out = pp->d_ro_rc[field_id];
    return VDF_OK;
  }
  const std::vector<Fe>& k = pp->ro->rc[field_id];
  const std::vector<Fe>& m = pp->ro->mds[field_id];
  { int rc = upload(pp->d_ro_block[field_id][0], k.data(), k.size() * sizeof(Fe)); if (rc != VDF_OK) return rc; }
  { int rc = upload(pp->d_ro_block[field_id][1], m.data(), m.size() * sizeof(Fe)); if (rc != VDF_OK) return rc; }
  *rc_out = pp->d_ro_block[field_id][0];
  *mds_out = pp->d_ro_block[field_id][1];
  return VDF_OK;
}
static_assert(offsetof(RoConstants, in) == RO_RF * RO_T * sizeof(Fe) && RO_RF * RO_T + RO_RP == VDF_RO_CONSTANTS,
              "RoConstants begins with the 88 constants in the order vdf_ro_hash_batch reads them");

// exact_checks with the three Poseidon hashes of every entry made by vdf_ro_hash_batch (the default block) or
// vdf_ro_hash_batch_block (any other): a host pass
// packs the messages of hash_state (both sides) and hash_challenge into one pinned block the kernel reads in place, three
// launches and one wait follow, and the comparisons run on the host in entry order.  *first_bad is exact_checks' value for
// every input: the entries in front of the first structural failure are hashed and compared, so an earlier mismatch wins.
template <class Passed>
int exact_checks_ro_device(const vdf_aggregate* agg, vdf_pp* pp, size_t count, const size_t num_steps[], const vdf_fe* z0, const vdf_fe* zi,
                           int64_t* first_bad, Passed&& passed) {
  const Side& S1 = pp->s[PRIMARY];
  const Side& S2 = pp->s[SECONDARY];
  const Field& F1 = *S1.F;
  const Field& F2 = *S2.F;
  const size_t ar = pp->arity;
  vdf_ctx* ctx = pp->ctx;
  *first_bad = -1;
  size_t live = count;                                     // the entries in front of the first structural failure
  for (size_t k = 0; k < count; ++k)
    if (agg->st[k].zi1.size() != ar) { live = k; *first_bad = (int64_t)k; break; }
  if (live == 0) return VDF_OK;
  const size_t len1 = 2 + 2 * ar + 9, len2 = 13, len3 = 16;
  void* blk = nullptr;
  HIPCALL(ctx, vdf_host_alloc(ctx, live * (len1 + len2 + len3 + 3) * sizeof(Fe), &blk));
  struct Free { vdf_ctx* c; void* p; ~Free() { vdf_host_free(c, p); } } free_blk{ctx, blk};
  Fe* m1 = static_cast<Fe*>(blk);
  Fe* m2 = m1 + live * len1;
  Fe* m3 = m2 + live * len2;
  Fe* h1 = m3 + live * len3;                               // plain integers: 250, 250 and 128 bits
  Fe* h2 = h1 + live;
  Fe* h3 = h2 + live;
  for (size_t k = 0; k < live; ++k) {
    const vdf_aggregate::Statement& s = agg->st[k];
    const RelaxedInst U2 = to_relaxed(s.r_U2, F2), U1 = to_relaxed(s.r_U1, F1);
    Fe* x = m1 + k * len1;                                 // hash_state over S1.field: params, i, z0, zi, the running secondary instance
    x[0] = pp->params[PRIMARY];
    x[1] = from_u64(num_steps[k], F1);
    memcpy(x + 2, (const Fe*)z0 + k * ar, ar * sizeof(Fe));
    memcpy(x + 2 + ar, s.zi1.data(), ar * sizeof(Fe));
    relaxed_elements(U2, F1, x + 2 + 2 * ar);
    x = m2 + k * len2;                                     // hash_state over S2.field: z0 = (0), zi = (zi2), the running primary instance
    x[0] = pp->params[SECONDARY];
    x[1] = from_u64(num_steps[k], F2);
    x[2] = zero();
    x[3] = s.zi2;
    relaxed_elements(U1, F2, x + 4);
    x = m3 + k * len3;                                     // hash_challenge over S1.field (fold_challenge)
    x[0] = pp->params[PRIMARY];
    relaxed_elements(U2, F1, x + 1);
    x[10] = s.l_u2.comm_W.x; x[11] = s.l_u2.comm_W.y;
    for (int j = 0; j < 2; ++j) { uint64_t ux[4]; fe_to_int(s.l_u2.X[j], F2, ux); x[12 + j] = int_to_fe(ux, F1); }
    x[14] = s.T2.x; x[15] = s.T2.y;
  }
  const void *rc1 = nullptr, *rc2 = nullptr, *mds1 = nullptr, *mds2 = nullptr;
  { int rc = ro_constants_on_device(pp, S1.field, &rc1, &mds1); if (rc != VDF_OK) return rc; }
  { int rc = ro_constants_on_device(pp, S2.field, &rc2, &mds2); if (rc != VDF_OK) return rc; }
  const RoSpec& sp = pp->ro->spec;
  // one launch: the family-0 kernel for the default block, the block kernel for any other
  auto hash = [&](int f, uint64_t tag, const void* rc, const void* mds, const Fe* xs, size_t len, int bits, Fe* out) -> int {
    return pp->ro->is_default
               ? vdf_ro_hash_batch(ctx, f, tag, (const vdf_fe*)rc, (const vdf_fe*)xs, len, live, bits, (vdf_fe*)out)
               : vdf_ro_hash_batch_block(ctx, f, tag, sp.width, sp.full_rounds, sp.partial_rounds, (const vdf_fe*)rc, (const vdf_fe*)mds,
                                         (const vdf_fe*)xs, len, live, bits, (vdf_fe*)out);
  };
  {
    AsyncScope scope(ctx);
    { int rc = scope.enter(); if (rc != VDF_OK) return rc; }
    HIPCALL(ctx, hash(S1.field, TAG_STATE, rc1, mds1, m1, len1, HASH_BITS, h1));
    HIPCALL(ctx, hash(S2.field, TAG_STATE, rc2, mds2, m2, len2, HASH_BITS, h2));
    HIPCALL(ctx, hash(S1.field, TAG_CHAL, rc1, mds1, m3, len3, CHAL_BITS, h3));
    HIPCALL(ctx, vdf_ctx_sync(ctx));
  }
  pp->verify_ro_stats[0] += 3 * live;
  pp->verify_ro_stats[1] += 3;
  for (size_t k = 0; k < live; ++k) {
    const vdf_aggregate::Statement& s = agg->st[k];
    if (int_to_fe(h1[k].l, F2) != s.l_u2.X[0] || int_to_fe(h2[k].l, F2) != s.l_u2.X[1] ||
        memcmp(s.zi1.data(), (const Fe*)zi + k * ar, 32 * ar) != 0 || !s.zi2.is_zero()) {
      *first_bad = (int64_t)k;
      return VDF_OK;
    }
    passed(k, s, h3[k].l);
  }
  return VDF_OK;
}

// Both arguments against the two accumulators (the unchanged spartan_replay / ipa_check_one): *ok = 1 when they hold.  The
// context is switched to asynchronous calls for the replay and put back as it was.
int check_arguments(const vdf_aggregate* agg, vdf_pp* pp, const Inst acc[2], int* ok) {
  vdf_ctx* ctx = pp->ctx;
  int was_async = 0;
  HIPCALL(ctx, vdf_ctx_get_async(ctx, &was_async));
  HIPCALL(ctx, vdf_ctx_sync(ctx));
  HIPCALL(ctx, vdf_ctx_set_async(ctx, 1));
  struct Restore { vdf_ctx* c; int a; ~Restore() { vdf_ctx_sync(c); vdf_ctx_set_async(c, a); } } restore{ctx, was_async};
  for (int side = 0; side < 2; ++side) {
    const Side& sd = pp->s[side];
    IpaDeferred d[2];
    bool good = false;
    int rc = spartan_replay(sd, acc[side].comm_W, acc[side].comm_E, acc[side].u, acc[side].X, agg->sp[side], d, &good);
    if (rc != VDF_OK || !good) return rc;
    DevBufs bufs(sd.ctx, sd.arena);
    const size_t n = std::max(d[0].n, d[1].n);
    void* d_s;
    { int rc2 = bufs.reserve(n); if (rc2 != VDF_OK) return fail(rc2, vdf_last_error(sd.ctx)); }
    { int rc2 = bufs.zeros(n, &d_s); if (rc2 != VDF_OK) return fail(rc2, vdf_last_error(sd.ctx)); }
    for (int q = 0; q < 2; ++q) {
      rc = ipa_check_one(sd, d[q], d_s, &good);
      if (rc != VDF_OK || !good) return rc;
    }
  }
  *ok = 1;
  return VDF_OK;
}

// fold_instances_core with the group arithmetic on the device.  No challenge depends on a folded accumulator (every instance is
// absorbed before the first one, then only commit(TT_k)), so the K - 1 sequential folds of the commitments are two sums,
//   comm_W = W_1 + sum_{k>=2} r_k W_k          comm_E = E_1 + sum_{k>=2} (r_k^2 E_k + r_k TT_k),
// one vdf_msm_batch of two vectors over the 3K - 1 points [W_1..W_K | E_1..E_K | TT_2..TT_K] uploaded as they are (no table: the
// bucket method takes equal points, opposite points and the identity, msm.hip k_accumulate).  The transcript, the challenges and
// the folds of u and X stay on the host.  packed: those points in that order in memory a copy can read (a device or pinned
// block the decoder wrote), or null: they are gathered from inst and TT.  sd: a side of the parameter set (ctx, curve, F, Fb, digest).
int fold_instances_on_device(const Side& sd, int side, size_t count, const Inst* inst, const Aff* TT, const vdf_affine* packed, Inst* acc,
                             Fe* r_out) {
  const Field& F = *sd.F;
  const Field& Fb = *sd.Fb;
  vdf_ctx* ctx = sd.ctx;
  Transcript tr("aggregate");
  const uint64_t head[2] = {(uint64_t)count, (uint64_t)side};
  tr.absorb("count", head, 16);
  for (size_t k = 0; k < count; ++k) instance_bytes(tr, sd, inst[k].comm_W, inst[k].comm_E, inst[k].u, inst[k].X);
  Inst a = inst[0];
  if (count == 1) { *acc = a; return VDF_OK; }
  std::vector<Fe> sw(count), se(2 * count - 1);
  sw[0] = se[0] = one(F);
  for (size_t k = 1; k < count; ++k) {
    tr.absorb_pt("T", &TT[k - 1], 1, Fb);
    uint64_t raw[4];
    const Fe r = tr.challenge("r", F, raw);
    sw[k] = r;
    se[k] = sqr(r, F);
    se[count + k - 1] = r;
    a.u = add(a.u, mul(r, inst[k].u, F), F);
    for (int j = 0; j < NUM_IO; ++j) a.X[j] = add(a.X[j], mul(r, inst[k].X[j], F), F);
    if (r_out) r_out[k - 1] = r;
  }
  std::vector<Aff> own;
  if (!packed) {
    own.resize(3 * count - 1);
    for (size_t k = 0; k < count; ++k) { own[k] = inst[k].comm_W; own[count + k] = inst[k].comm_E; }
    for (size_t k = 0; k + 1 < count; ++k) own[2 * count + k] = TT[k];
    packed = (const vdf_affine*)own.data();
  }
  vdf_bases* pb = nullptr;
  HIPCALL(ctx, vdf_bases_upload(ctx, sd.curve, packed, 3 * count - 1, &pb));
  const size_t off[2] = {0, count}, n[2] = {count, 2 * count - 1};
  const vdf_fe* const sc[2] = {(const vdf_fe*)sw.data(), (const vdf_fe*)se.data()};
  vdf_jac j[2];
  int rc = vdf_msm_batch(ctx, pb, 2, off, sc, n, 1, j);
  if (rc == VDF_OK) rc = vdf_ctx_sync(ctx);
  const std::string err = rc == VDF_OK ? "" : vdf_last_error(ctx);
  vdf_bases_free(pb);
  if (rc != VDF_OK) return fail(rc, "vdf_msm_batch (aggregate fold): " + err);
  jac_to_aff2(j[0], j[1], Fb, &a.comm_W, &a.comm_E);
  *acc = a;
  return VDF_OK;
}

// n 32-byte encodings of one curve decoded by one vdf_points_decompress on a pinned block the kernel reads and writes in place
// (compress_host.cpp's wire batch has the same block): [enc: 32 n | points: 64 n | ok: n].  The caller fills enc(), decodes
// and reads points() / good() after a wait; the block is a device address too, so the points can go on to an upload as they lie.
struct DecodeBlock {
  vdf_ctx* ctx;
  size_t n;
  void* blk = nullptr;
  DecodeBlock(vdf_ctx* c, size_t n_) : ctx(c), n(n_) {}
  ~DecodeBlock() { if (blk) vdf_host_free(ctx, blk); }
  int alloc() { return vdf_host_alloc(ctx, 97 * n, &blk); }
  uint8_t* enc() { return static_cast<uint8_t*>(blk); }
  vdf_affine* points() { return reinterpret_cast<vdf_affine*>(enc() + 32 * n); }
  const uint8_t* good() { return enc() + 96 * n; }
};

// what the last device verification of this thread spent where, in ms (vdf_nova_aggregate_verify_times)
thread_local double g_verify_ms[5] = {0, 0, 0, 0, 0};

}  // namespace

extern "C" {

int vdf_nova_compress_aggregate(vdf_pp* pp, size_t count, const vdf_proof* const proofs[], vdf_aggregate** out) {
  return nova_guard([&]() -> int {
    if (!pp || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (count == 0 || count > VDF_NOVA_AGGREGATE_MAX) return fail(VDF_ERR_BAD_ARG, "count must be 1.." + std::to_string(VDF_NOVA_AGGREGATE_MAX));
    if (!proofs) return fail(VDF_ERR_BAD_ARG, "null argument");
    for (size_t q = 0; q < count; ++q) {
      const vdf_proof* p = proofs[q];
      if (!p) return fail(VDF_ERR_BAD_ARG, "entry " + std::to_string(q) + ": null proof");
      if (p->pp != pp) return fail(VDF_ERR_BAD_ARG, "entry " + std::to_string(q) + ": proof was made under other public parameters");
      if (p->i == 0) return fail(VDF_ERR_BAD_LENGTH, "entry " + std::to_string(q) + ": nothing to compress");
    }
    for (size_t q = 0; q < count; ++q) { int rc = finalize_l2(proofs[q]); if (rc != VDF_OK) return rc; }
    vdf_ctx* ctx = pp->ctx;
    const Side& S1 = pp->s[PRIMARY];
    const Side& S2 = pp->s[SECONDARY];
    int was_async = 0;
    HIPCALL(ctx, vdf_ctx_get_async(ctx, &was_async));
    HIPCALL(ctx, vdf_ctx_sync(ctx));
    HIPCALL(ctx, vdf_ctx_set_async(ctx, 1));
    struct Restore { vdf_ctx* c; int a; ~Restore() { vdf_ctx_sync(c); vdf_ctx_set_async(c, a); } } restore{ctx, was_async};
    std::unique_ptr<vdf_aggregate> a(new vdf_aggregate());
    a->t = pp->t;
    a->field = pp->field;
    a->arity = pp->arity;
    memcpy(a->digest, pp->digest, 32);
    a->st.resize(count);
    const bool folds = count > 1;
    // device scratch: one accumulator per side and one incoming folded secondary instance, whatever the count
    DevBufs bufs(ctx);
    SideFold f1(S1, ctx), f2(S2, ctx);
    { int rc = f1.alloc(bufs, folds); if (rc != VDF_OK) return rc; }
    { int rc = f2.alloc(bufs, folds); if (rc != VDF_OK) return rc; }
    void *d_fz, *d_fE;
    { int rc = bufs.zeros(S2.ncols, &d_fz); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    { int rc = bufs.zeros(S2.num_cons, &d_fE); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    // Every instance is absorbed before the first challenge of its side, and a secondary instance F2_k is the result of a
    // prelude: the preludes run first, entry by entry.  Each leaves its cross term T2_k in the proof's own secondary scratch
    // vector, so the folded witness of an entry is two vdf_axpy away when its turn to be folded comes.
    std::vector<Inst> i1(count), i2(count);
    for (size_t q = 0; q < count; ++q) {
      vdf_snark s;
      { int rc = compress_prelude(proofs[q], pp, &s, d_fz, d_fE, &i2[q]); if (rc != VDF_OK) return rc; }
      vdf_aggregate::Statement& st = a->st[q];
      st.r_U1 = s.r_U1; st.r_U2 = s.r_U2; st.l_u2 = s.l_u2; st.T2 = s.T2; st.zi1 = s.zi1; st.zi2 = s.zi2[0];
      i1[q] = s.r_U1;
    }
    f1.start(count, i1.data());
    f2.start(count, i2.data());
    a->TT[0].resize(count - 1);
    a->TT[1].resize(count - 1);
    for (size_t q = 0; q < count; ++q) {
      const vdf_proof* p = proofs[q];
      Aff tt;
      { int rc = f1.take(i1[q], p->r[PRIMARY].d_z, p->r[PRIMARY].d_E, folds, &tt); if (rc != VDF_OK) return rc; }
      if (q) a->TT[0][q - 1] = tt;
      if (folds) {                                     // (a single entry's folded witness is where its prelude left it)
        const vdf_aggregate::Statement& st = a->st[q];
        const SideState& s2 = p->r[SECONDARY];
        uint64_t r[4];
        fold_challenge(pp, st.r_U2, st.l_u2, st.T2, r);
        const Fe rf = int_to_fe(r, *S2.F);
        HIPCALL(ctx, vdf_axpy(ctx, S2.field, (const vdf_fe*)s2.d_z, (const vdf_fe*)&rf, (const vdf_fe*)p->d_l2z, S2.ncols, (vdf_fe*)d_fz));
        HIPCALL(ctx, vdf_axpy(ctx, S2.field, (const vdf_fe*)s2.d_E, (const vdf_fe*)&rf, (const vdf_fe*)s2.d_T, S2.num_cons, (vdf_fe*)d_fE));
      }
      { int rc = f2.take(i2[q], d_fz, d_fE, folds, &tt); if (rc != VDF_OK) return rc; }
      if (q) a->TT[1][q - 1] = tt;
    }
    std::lock_guard<std::mutex> aux_lock(pp->aux_mu);
    const ProveIn in1{f1.inst.comm_W, f1.inst.comm_E, f1.inst.u, f1.inst.X, f1.z, f1.E, &a->sp[0]};
    const ProveIn in2{f2.inst.comm_W, f2.inst.comm_E, f2.inst.u, f2.inst.X, f2.z, f2.E, &a->sp[1]};
    { int rc = prove_both_sides(pp, 1, &in1, &in2, &pp->arena[PRIMARY], &pp->arena[SECONDARY]); if (rc != VDF_OK) return rc; }
    *out = a.release();
    return VDF_OK;
  });
}

void vdf_nova_aggregate_free(vdf_aggregate* agg) { delete agg; }
size_t vdf_nova_aggregate_count(const vdf_aggregate* agg) { return agg ? agg->st.size() : 0; }

int vdf_nova_aggregate_fold_instances(int field_of_primary, int side, const uint8_t digest[32], size_t count, const vdf_wire_instance inst[],
                                      const uint8_t comm_TT[][32], vdf_wire_instance* acc, vdf_fe r_out[]) {
  return nova_guard([&]() -> int {
    if (!valid_field(field_of_primary) || (side != 0 && side != 1)) return fail(VDF_ERR_BAD_ARG, "unknown field or side");
    if (!digest || !inst || !acc || (count > 1 && !comm_TT)) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (count == 0 || count > VDF_NOVA_AGGREGATE_MAX) return fail(VDF_ERR_BAD_ARG, "count must be 1.." + std::to_string(VDF_NOVA_AGGREGATE_MAX));
    const Side sd = host_side(field_of_primary, side, digest);
    std::vector<Inst> in(count);
    std::vector<Aff> tt(count - 1);
    bool canonical = true, on_curve = true;
    for (size_t k = 0; k < count; ++k) get_inst(reinterpret_cast<const uint8_t*>(&inst[k]), &in[k], sd, true, &canonical, &on_curve);
    for (size_t k = 0; k + 1 < count; ++k) on_curve &= pt_decompress(comm_TT[k], *sd.Fb, &tt[k]);
    if (!canonical) return fail(VDF_ERR_NONCANONICAL, "a field element of an instance is not canonical");
    if (!on_curve) return fail(VDF_ERR_NONCANONICAL, "a point does not decode to a curve point");
    Inst folded;
    fold_instances_core(sd, side, count, in.data(), tt.data(), &folded, reinterpret_cast<Fe*>(r_out));
    put_inst(reinterpret_cast<uint8_t*>(acc), folded, sd, true);
    return VDF_OK;
  });
}

int vdf_nova_verify_aggregate(const vdf_aggregate* agg, vdf_pp* pp, size_t count, const size_t num_steps[], const vdf_fe* z0, const vdf_fe* zi,
                              int* ok, int64_t* bad_entry) {
  return nova_guard([&]() -> int {
    if (!agg || !pp || !ok) return fail(VDF_ERR_BAD_ARG, "null argument");
    *ok = 0;
    if (bad_entry) *bad_entry = -1;
    if (agg->t != pp->t || memcmp(agg->digest, pp->digest, 32) != 0) return fail(VDF_ERR_BAD_ARG, "aggregate was made under other public parameters");
    if (count == 0 || count != agg->st.size()) return VDF_OK;
    if (!num_steps || !z0 || !zi) return fail(VDF_ERR_BAD_ARG, "null argument");
    const Side& S1 = pp->s[PRIMARY];
    const Side& S2 = pp->s[SECONDARY];
    auto bad = [&](size_t k) { if (bad_entry) *bad_entry = (int64_t)k; return VDF_OK; };
    for (size_t k = 0; k < count; ++k) if (num_steps[k] == 0) return bad(k);
    // the exact checks of every entry, then the verifier's own secondary fold
    std::vector<Inst> i1(count), i2(count);
    const int64_t first_bad = exact_checks(agg, pp, count, num_steps, z0, zi, [&](size_t k, const vdf_aggregate::Statement& s, const uint64_t r[4]) {
      i1[k] = s.r_U1;
      i2[k] = fold_instance(S2, s.r_U2, s.l_u2, s.T2, r);
    });
    if (first_bad >= 0) return bad((size_t)first_bad);
    if (agg->TT[0].size() != count - 1 || agg->TT[1].size() != count - 1) return VDF_OK;
    Inst acc[2];
    fold_instances_core(S1, PRIMARY, count, i1.data(), agg->TT[0].data(), &acc[0], nullptr);
    fold_instances_core(S2, SECONDARY, count, i2.data(), agg->TT[1].data(), &acc[1], nullptr);
    return check_arguments(agg, pp, acc, ok);
  });
}

// ---- "VDFAGG01" (layout in include/vdf_nova.h) ---------------------------------------------------------------------------------
size_t vdf_nova_aggregate_serialized_size(const vdf_aggregate* agg) {
  if (!agg || agg->st.empty()) return 0;
  size_t n = AGG_HEADER + agg->st.size() * statement_wire(agg->arity) + 2 * (agg->st.size() - 1) * 32;
  for (const Spartan& p : agg->sp)
    n += 32 * (3 * p.outer.size() + 4 + 2 * p.inner.size() + 1 + p.ipaW.a.size() + p.ipaE.a.size()) + 64 * (p.ipaW.L.size() + p.ipaE.L.size());
  return n;
}

int vdf_nova_aggregate_serialize(const vdf_aggregate* agg, uint8_t* out, size_t cap) {
  return nova_guard([&]() -> int {
    if (!agg || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (cap < vdf_nova_aggregate_serialized_size(agg)) return fail(VDF_ERR_BAD_LENGTH, "buffer too small");
    const Side sd[2] = {host_side(agg->field, 0, agg->digest), host_side(agg->field, 1, agg->digest)};
    uint8_t* o = out;
    memcpy(o, WIRE_MAGIC_AGGREGATE, 8); o += 8;
    memcpy(o, &agg->t, 8); o += 8;
    const uint64_t count = agg->st.size();
    memcpy(o, &count, 8); o += 8;
    memcpy(o, agg->digest, 32); o += 32;
    for (const vdf_aggregate::Statement& s : agg->st) {
      o = put_inst(o, s.r_U1, sd[0], true);
      o = put_inst(o, s.r_U2, sd[1], true);
      o = put_inst(o, s.l_u2, sd[1], false);
      pt_compress(s.T2, *sd[1].Fb, o); o += 32;
      for (const Fe& v : s.zi1) o = wire_put_fe(o, v, *sd[0].F);
      o = wire_put_fe(o, s.zi2, *sd[1].F);
    }
    for (int side = 0; side < 2; ++side)
      for (const Aff& p : agg->TT[side]) { pt_compress(p, *sd[side].Fb, o); o += 32; }
    for (int side = 0; side < 2; ++side) o = put_argument(o, agg->sp[side], *sd[side].F, *sd[side].Fb);
    return VDF_OK;
  });
}

int vdf_nova_aggregate_deserialize(vdf_pp* pp, const uint8_t* in, size_t len, vdf_aggregate** out) {
  return nova_guard([&]() -> int {
    if (!pp || !in || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    Layout L[2];
    size_t count = 0;
    { int rc = aggregate_wire_header(pp, in, len, L, &count); if (rc != VDF_OK) return rc; }
    bool canonical = true, on_curve = true;
    std::unique_ptr<vdf_aggregate> a = aggregate_wire_walk(pp, L, in, count, &canonical, [&](const uint8_t* enc, const Side& sd, Aff* dst) {
      on_curve &= pt_decompress(enc, *sd.Fb, dst);
    });
    if (!canonical) return fail(VDF_ERR_NONCANONICAL, "a field element of the encoding is not canonical");
    if (!on_curve) return fail(VDF_ERR_NONCANONICAL, "a point of the encoding does not decode to a curve point");
    *out = a.release();
    return VDF_OK;
  });
}

// ---- the verifier with its per-entry group arithmetic on the device -------------------------------------------------------------
int vdf_nova_aggregate_fold_instances_device(vdf_pp* pp, int side, size_t count, const vdf_wire_instance inst[], const uint8_t comm_TT[][32],
                                             vdf_wire_instance* acc, vdf_fe r_out[]) {
  return nova_guard([&]() -> int {
    if (!pp) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (side != 0 && side != 1) return fail(VDF_ERR_BAD_ARG, "unknown field or side");
    if (!inst || !acc || (count > 1 && !comm_TT)) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (count == 0 || count > VDF_NOVA_AGGREGATE_MAX) return fail(VDF_ERR_BAD_ARG, "count must be 1.." + std::to_string(VDF_NOVA_AGGREGATE_MAX));
    const Side& sd = pp->s[side];
    vdf_ctx* ctx = sd.ctx;
    std::vector<Inst> in(count);
    bool canonical = true;
    for (size_t k = 0; k < count; ++k) {
      canonical &= wire_get_fe(inst[k].u, *sd.F, &in[k].u);
      for (int j = 0; j < NUM_IO; ++j) canonical &= wire_get_fe(inst[k].X[j], *sd.F, &in[k].X[j]);
    }
    if (!canonical) return fail(VDF_ERR_NONCANONICAL, "a field element of an instance is not canonical");
    // the 3 count - 1 encodings in the order the sums take their points: [W_1..W_K | E_1..E_K | TT_2..TT_K]
    const size_t np = 3 * count - 1;
    DecodeBlock blk(ctx, np);
    HIPCALL(ctx, blk.alloc());
    for (size_t k = 0; k < count; ++k) {
      memcpy(blk.enc() + 32 * k, inst[k].comm_W, 32);
      memcpy(blk.enc() + 32 * (count + k), inst[k].comm_E, 32);
    }
    for (size_t k = 0; k + 1 < count; ++k) memcpy(blk.enc() + 32 * (2 * count + k), comm_TT[k], 32);
    AsyncScope scope(ctx);
    { int rc = scope.enter(); if (rc != VDF_OK) return rc; }
    HIPCALL(ctx, vdf_points_decompress(ctx, sd.curve, blk.enc(), np, blk.points(), const_cast<uint8_t*>(blk.good())));
    HIPCALL(ctx, vdf_ctx_sync(ctx));
    for (size_t k = 0; k < np; ++k)
      if (!blk.good()[k]) return fail(VDF_ERR_NONCANONICAL, "a point does not decode to a curve point");
    const Aff* pts = reinterpret_cast<const Aff*>(blk.points());
    for (size_t k = 0; k < count; ++k) { in[k].comm_W = pts[k]; in[k].comm_E = pts[count + k]; }
    Inst folded;
    { int rc = fold_instances_on_device(sd, side, count, in.data(), pts + 2 * count, blk.points(), &folded, reinterpret_cast<Fe*>(r_out)); if (rc != VDF_OK) return rc; }
    put_inst(reinterpret_cast<uint8_t*>(acc), folded, sd, true);
    return VDF_OK;
  });
}

int vdf_nova_verify_aggregate_device(const vdf_aggregate* agg, vdf_pp* pp, size_t count, const size_t num_steps[], const vdf_fe* z0,
                                     const vdf_fe* zi, int* ok, int64_t* bad_entry) {
  return nova_guard([&]() -> int {
    if (!agg || !pp || !ok) return fail(VDF_ERR_BAD_ARG, "null argument");
    *ok = 0;
    if (bad_entry) *bad_entry = -1;
    if (agg->t != pp->t || memcmp(agg->digest, pp->digest, 32) != 0) return fail(VDF_ERR_BAD_ARG, "aggregate was made under other public parameters");
    if (count == 0 || count != agg->st.size()) return VDF_OK;
    if (!num_steps || !z0 || !zi) return fail(VDF_ERR_BAD_ARG, "null argument");
    const Side& S1 = pp->s[PRIMARY];
    const Side& S2 = pp->s[SECONDARY];
    const Field& F2 = *S2.F;
    auto bad = [&](size_t k) { if (bad_entry) *bad_entry = (int64_t)k; return VDF_OK; };
    for (size_t k = 0; k < count; ++k) if (num_steps[k] == 0) return bad(k);
    for (double& v : g_verify_ms) v = 0;
    double t0 = now_ms();
    // the exact checks of every entry on the host; of the verifier's own secondary fold only the challenge, u and X
    std::vector<Inst> i1(count), i2(count);
    std::vector<Aff> fa(2 * count), fb(2 * count), fo(2 * count);          // [comm_W of every entry | comm_E of every entry]
    std::vector<Fe> rho(2 * count);
    auto passed = [&](size_t k, const vdf_aggregate::Statement& s, const uint64_t r[4]) {
      i1[k] = s.r_U1;
      const Fe rf = int_to_fe(r, F2);
      i2[k].u = add(s.r_U2.u, rf, F2);
      for (int j = 0; j < NUM_IO; ++j) i2[k].X[j] = add(s.r_U2.X[j], mul(rf, s.l_u2.X[j], F2), F2);
      fa[k] = s.r_U2.comm_W; fb[k] = s.l_u2.comm_W;
      fa[count + k] = s.r_U2.comm_E; fb[count + k] = s.T2;
      memcpy(rho[k].l, r, 32);
      rho[count + k] = rho[k];
    };
    // the three Poseidon hashes of every entry: on the host, or by vdf_ro_hash_batch under the default block
    // (vdf_nova_pp_set_verify_ro_device), or by vdf_ro_hash_batch_block under another block (vdf_nova_pp_set_verify_ro_block_device)
    const int ro_min = pp->ro->is_default ? pp->verify_ro_device.load() : pp->verify_ro_block_device.load();
    int64_t first_bad = -1;
    if (ro_min > 0 && count >= (size_t)ro_min) {
      int rc = exact_checks_ro_device(agg, pp, count, num_steps, z0, zi, &first_bad, passed);
      if (rc != VDF_OK) return rc;
    } else {
      first_bad = exact_checks(agg, pp, count, num_steps, z0, zi, passed);
    }
    g_verify_ms[0] = now_ms() - t0;
    if (first_bad >= 0) return bad((size_t)first_bad);
    if (agg->TT[0].size() != count - 1 || agg->TT[1].size() != count - 1) return VDF_OK;
    Inst acc[2];
    {
      vdf_ctx* ctx = pp->ctx;
      AsyncScope scope(ctx);
      { int rc = scope.enter(); if (rc != VDF_OK) return rc; }
      t0 = now_ms();
      // F2_k = r_U2_k + rho_k l_u2_k: comm_W = W_r + rho W_l, comm_E = E_r + rho T2 (rho: the 128-bit Poseidon challenge)
      HIPCALL(ctx, vdf_points_axpy(ctx, S2.curve, (const vdf_affine*)fa.data(), (const vdf_affine*)fb.data(), (const vdf_fe*)rho.data(), 128,
                                   2 * count, (vdf_affine*)fo.data()));
      for (size_t k = 0; k < count; ++k) { i2[k].comm_W = fo[k]; i2[k].comm_E = fo[count + k]; }
      g_verify_ms[1] = now_ms() - t0;
      t0 = now_ms();
      { int rc = fold_instances_on_device(S1, PRIMARY, count, i1.data(), agg->TT[0].data(), nullptr, &acc[0], nullptr); if (rc != VDF_OK) return rc; }
      { int rc = fold_instances_on_device(S2, SECONDARY, count, i2.data(), agg->TT[1].data(), nullptr, &acc[1], nullptr); if (rc != VDF_OK) return rc; }
      g_verify_ms[2] = now_ms() - t0;
    }
    t0 = now_ms();
    const int rc = check_arguments(agg, pp, acc, ok);
    g_verify_ms[3] = now_ms() - t0;
    return rc;
  });
}

int vdf_nova_pp_set_verify_ro_device(vdf_pp* pp, int min_count) {
  if (!pp) return fail(VDF_ERR_BAD_ARG, "null argument");
  if (min_count < 0) return fail(VDF_ERR_BAD_ARG, "min_count must be 0 (never) or a positive count");
  pp->verify_ro_device.store(min_count);
  return VDF_OK;
}
int vdf_nova_pp_verify_ro_device(const vdf_pp* pp) { return pp ? pp->verify_ro_device.load() : 0; }
int vdf_nova_pp_set_verify_ro_block_device(vdf_pp* pp, int min_count) {
  if (!pp) return fail(VDF_ERR_BAD_ARG, "null argument");
  if (min_count < 0) return fail(VDF_ERR_BAD_ARG, "min_count must be 0 (never) or a positive count");
  pp->verify_ro_block_device.store(min_count);
  return VDF_OK;
}
int vdf_nova_pp_verify_ro_block_device(const vdf_pp* pp) { return pp ? pp->verify_ro_block_device.load() : 0; }
int vdf_nova_pp_verify_ro_stats(const vdf_pp* pp, uint64_t out[2]) {
  if (!pp || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
  for (int k = 0; k < 2; ++k) out[k] = pp->verify_ro_stats[k].load();
  return VDF_OK;
}

int vdf_nova_aggregate_verify_times(double ms[5]) {
  if (!ms) return fail(VDF_ERR_BAD_ARG, "null argument");
  for (int k = 0; k < 5; ++k) ms[k] = g_verify_ms[k];
  return VDF_OK;
}

int vdf_nova_verify_aggregate_wire(vdf_pp* pp, const uint8_t* bytes, size_t len, size_t count, const size_t num_steps[], const vdf_fe* z0,
                                   const vdf_fe* zi, int* ok, int64_t* bad_entry, int* decode_code) {
  return nova_guard([&]() -> int {
    if (!pp || !bytes || !ok || !decode_code) return fail(VDF_ERR_BAD_ARG, "null argument");
    *ok = 0;
    if (bad_entry) *bad_entry = -1;
    *decode_code = VDF_OK;
    const double t_decode = now_ms();
    Layout L[2];
    size_t wire_count = 0;
    *decode_code = aggregate_wire_header(pp, bytes, len, L, &wire_count);
    if (*decode_code != VDF_OK) return VDF_OK;
    struct WirePoint { const uint8_t* enc; Aff* dst; };
    std::vector<WirePoint> pts[2];
    bool canonical = true;
    std::unique_ptr<vdf_aggregate> a = aggregate_wire_walk(pp, L, bytes, wire_count, &canonical, [&](const uint8_t* enc, const Side& sd, Aff* dst) {
      pts[&sd - pp->s].push_back({enc, dst});
    });
    if (!canonical) { *decode_code = fail(VDF_ERR_NONCANONICAL, "a field element of the encoding is not canonical"); return VDF_OK; }
    {
      vdf_ctx* ctx = pp->ctx;
      const size_t n[2] = {pts[0].size(), pts[1].size()}, total = n[0] + n[1];
      DecodeBlock blk(ctx, total);                       // side 0's share of each part first
      HIPCALL(ctx, blk.alloc());
      {
        uint8_t* e = blk.enc();
        for (int side = 0; side < 2; ++side)
          for (const WirePoint& w : pts[side]) { memcpy(e, w.enc, 32); e += 32; }
      }
      {
        AsyncScope scope(ctx);
        { int rc = scope.enter(); if (rc != VDF_OK) return rc; }
        for (int side = 0; side < 2; ++side) {
          const size_t at = side ? n[0] : 0;
          HIPCALL(ctx, vdf_points_decompress(ctx, pp->s[side].curve, blk.enc() + 32 * at, n[side], blk.points() + at,
                                             const_cast<uint8_t*>(blk.good()) + at));
        }
        HIPCALL(ctx, vdf_ctx_sync(ctx));
      }
      for (size_t k = 0; k < total; ++k)
        if (!blk.good()[k]) {
          *decode_code = fail(VDF_ERR_NONCANONICAL, "a point of the encoding does not decode to a curve point");
          return VDF_OK;
        }
      size_t k = 0;
      for (int side = 0; side < 2; ++side)
        for (const WirePoint& w : pts[side]) memcpy(w.dst, &blk.points()[k++], sizeof(Aff));
    }
    const double decode_ms = now_ms() - t_decode;
    const int rc = vdf_nova_verify_aggregate_device(a.get(), pp, count, num_steps, z0, zi, ok, bad_entry);
    g_verify_ms[4] = decode_ms;
    return rc;
  });
}

}  // extern "C"
