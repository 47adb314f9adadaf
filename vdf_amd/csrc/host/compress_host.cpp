// libvdf_nova.so, part 3: NovaVDFProof::compress and verification of the compressed proof: one Spartan-style argument
// per side of the curve cycle (SS1 / SS2 of src/nova/proof.rs:32-33), after the last secondary instance is folded.
#include <algorithm>
#include <thread>
#include "nova_internal.hpp"

using namespace vdfnova;

// =============================================================================================================
// Compression SNARK: NovaVDFProof::compress / verification of the compressed proof (src/nova/proof.rs:360-368, :383).
// Protocol "vdf-spartan-v3", restated line by line by the test oracle (spartan.py: prove / verify); every pass over a vector is
// a call through include/vdf_hip.h, the host keeps the transcript, O(log n) field work and O(log n) point work.
// =============================================================================================================
namespace {

size_t pow2_at_least(size_t n) { size_t p = 1; while (p < n) p <<= 1; return p; }
int log2_exact(size_t n) { int k = 0; while (((size_t)1 << k) < n) ++k; return k; }

}  // namespace
namespace vdfnova {
Layout layout_of(const Side& pp_) {
  const Side* pp = &pp_;
  Layout l;
  l.M = pow2_at_least(pp->num_cons); l.NW = pow2_at_least(pp->num_vars); l.Z = 2 * l.NW;
  l.s = log2_exact(l.M); l.l1 = log2_exact(l.Z);
  return l;
}
}  // namespace vdfnova
namespace {

Fe small(uint64_t k, const Field& F) { return from_u64(k, F); }
// value at r of the polynomial through (0, y0), (1, y1), (2, y2)[, (3, y3)]
Fe interpolate(const Fe* y, int npts, const Fe& r, const Field& F) {
  Fe acc = zero();
  for (int i = 0; i < npts; ++i) {
    Fe num = one(F), den = one(F);
    for (int j = 0; j < npts; ++j)
      if (i != j) {
        num = mul(num, sub(r, small(j, F), F), F);
        den = mul(den, sub(small(i, F), small(j, F), F), F);
      }
    acc = add(acc, mul(y[i], mul(num, inverse(den, F), F), F), F);
  }
  return acc;
}

}  // namespace
namespace vdfnova {
void instance_bytes(Transcript& tr, const Side& sd, const Aff& cW, const Aff& cE, const Fe& u, const Fe* X) {
  const Field& F = *sd.F;
  tr.absorb("shape", sd.digest, 32);
  const Aff pts[2] = {cW, cE};
  tr.absorb_pt("inst", pts, 2, *sd.Fb);
  Fe v[1 + NUM_IO];
  v[0] = u;
  for (int j = 0; j < NUM_IO; ++j) v[1 + j] = X[j];
  tr.absorb_fe("inst", v, 1 + NUM_IO, F);
}
}  // namespace vdfnova
namespace {

// lo = 1 - r, hi = r table of eq(r, .) on the device
int eq_table_dev(const Side& sd, const std::vector<Fe>& r, void* out) {
  vdf_ctx* ctx = sd.ctx;
  const Field& F = *sd.F;
  std::vector<Fe> lo(r.size());
  for (size_t j = 0; j < r.size(); ++j) lo[j] = sub(one(F), r[j], F);
  HIPCALL(ctx, vdf_pair_table(ctx, sd.field, (const vdf_fe*)lo.data(), (const vdf_fe*)r.data(), (int)r.size(), (vdf_fe*)out));
  return VDF_OK;
}

// M(y) in the padded layout (W at [0, NW), u at NW, X after it) from eq(r_x, .)
int m_vector_dev(const Side& sd, const Layout& L, const void* d_eq_rx, const Fe& rho, void* d_cols, void* d_mvec) {
  const Side* pp = &sd;
  vdf_ctx* ctx = sd.ctx;
  HIPCALL(ctx, vdf_spmv3_t(ctx, pp->shape, (const vdf_fe*)d_eq_rx, (const vdf_fe*)&rho, (vdf_fe*)d_cols));
  HIPCALL(ctx, vdf_dev_memset(ctx, d_mvec, 0, L.Z * 32));
  HIPCALL(ctx, vdf_dev_memcpy(ctx, d_mvec, d_cols, pp->num_vars * 32));
  HIPCALL(ctx, vdf_dev_memcpy(ctx, (char*)d_mvec + L.NW * 32, (const char*)d_cols + pp->num_vars * 32, (1 + NUM_IO) * 32));
  return VDF_OK;
}

Pt pt_mul_fe(const Pt& p, const Fe& k_mont, const Field& Fscalar, const Field& Fb) {       // k in Montgomery form of the scalar field
  const Fe k = from_mont(k_mont, Fscalar);
  return pt_mul(p, k.l, 255, Fb);
}

// Fixed-base multiples of one point (the Q of an inner-product argument is multiplied by two fresh scalars per
// round): 4-bit windows, d * 16^w * Q for d = 1..15, so a product is 64 additions and no doubling.
struct FixedBase {
  std::vector<Pt> tab;            // [w * 15 + (d - 1)]
  const Field& Fb;
  FixedBase(const Pt& q, const Field& fb) : tab(64 * 15), Fb(fb) {
    Pt base = q;
    for (int w = 0; w < 64; ++w) {
      Pt acc = base;
      for (int d = 1; d <= 15; ++d) { tab[w * 15 + d - 1] = acc; acc = pt_add(acc, base, Fb); }
      base = acc;                  // 16 * base
    }
  }
  Pt mul(const Fe& k_mont, const Field& Fscalar) const {
    const Fe k = from_mont(k_mont, Fscalar);
    Pt r = pt_identity();
    for (int w = 0; w < 64; ++w) {
      const unsigned d = (unsigned)(k.l[w / 16] >> (4 * (w % 16))) & 15u;
      if (d) r = pt_add(r, tab[w * 15 + d - 1], Fb);
    }
    return r;
  }
};

// One opening <a, b> = v under P = <a, G[0..n)>: a, b, s are device vectors of length n that the argument consumes
// (s = all ones), sL / sR scratch of the same length.
struct IpaJob {
  const char* label;
  size_t n;
  void *d_a, *d_b, *d_s, *d_sL, *d_sR;
  Fe v;
  Aff P;
  Ipa* out;
  // state
  size_t nj = 0;
  uint64_t q_raw[4];               // the 128-bit challenge Q = q_raw * gen_u comes from
  Pt Qp;
  std::unique_ptr<FixedBase> Qtab;
  // Q and its table of 960 multiples (~0.15 ms of host work): wanted when the first round's points come back, not before
  void make_q(const Aff& gen_u, const Field& Fb) {
    Qp = pt_mul(pt_from_aff(gen_u, Fb), q_raw, 128, Fb);
    Qtab.reset(new FixedBase(Qp, Fb));
  }
  Fe* cross = nullptr;             // two elements in pinned, device-mapped memory: the reduction writes them in place and they are
                                   // read after the round's one synchronisation (behind the MSM), not after one of their own
};

// The rounds of many openings.  A UNIT is one or two openings of one transcript whose L and R go into ONE batched MSM per
// round (two or four groups: one sort, one accumulate grid, one bucket reduction) on the unit's queue; a unit's round ends
// with one wait (for its MSM's mark), then job by job its points are absorbed, its challenge drawn and its vectors folded,
// and its next round is enqueued at once -- before the next unit's points of this round are read.  Only launches move
// between units: every transcript sees what the test oracle's lockstep prover (ipa_prove_many) gives it -- round by round
// W's L, R and challenge, then E's -- so the bytes of a proof do not depend on how its openings are grouped.
//   * one proof, two queues: W and E are units of their own, half a round apart.  A round's batched MSM is sort (0.26 ms at
//     2^19 + 2^18 generators), bucket accumulation (0.91), fix-up and bucket reduction (0.26): only the middle one fills
//     the device, and in lockstep the device idles through the other two and through the host's turn, 15 times.  E's
//     accumulation is gated behind W's whole MSM (vdf_ctx_gate_accumulate): E's sort runs under W's accumulation, E's
//     accumulation under W's host turn and W's next sort, E's reduction under W's next accumulation.
//   * one proof, one queue: a single unit of both openings (the oracle's lockstep, one four-group MSM per round).
//   * K proofs (vdf_nova_compress_batch): a unit per proof, round robin over the side's queues, each unit's accumulation
//     gated behind the MSM of the unit enqueued just before it on another queue: one proof's sort, tail and host turn
//     run under another's accumulation.
constexpr int IPA_MARK = 8;                  // (library slots, vdf_hip.h: 0..3 on the caller's context are the caller's; prove_step holds 4..7)
constexpr int IPA_UNITS_PER_QUEUE = VDF_MARK_SLOTS - IPA_MARK;
struct IpaUnit {
  Transcript* tr;
  IpaJob* jobs[2];
  int njobs;
  vdf_ctx* ctx;                    // its queue
  int slot;                        // its mark slot on that queue
  vdf_jac* h_lr;                   // 2 * njobs pinned result points
};

int ipa_prove_units(const Side& sd, IpaUnit* units, int nunits) {
  const Side* pp = &sd;
  const Field& F = *sd.F;
  const Field& Fb = *sd.Fb;
  uint64_t raw[4];
  std::vector<vdf_ctx*> queues;
  for (int u = 0; u < nunits; ++u)
    if (std::find(queues.begin(), queues.end(), units[u].ctx) == queues.end()) queues.push_back(units[u].ctx);
  // whatever way this function is left, nothing of it is still on any queue: the caller frees the pinned result slots
  struct Drain { std::vector<vdf_ctx*>& q; ~Drain() { for (vdf_ctx* c : q) (void)vdf_ctx_sync(c); } } drain{queues};
  for (vdf_ctx* c : queues)
    if (c != sd.ctx) {
      HIPCALL(c, vdf_ctx_set_async(c, 1));
      HIPCALL(c, vdf_ctx_wait(c, sd.ctx));                            // the openings' vectors were made on the side's queue
    }
  for (int u = 0; u < nunits; ++u)
    for (int j = 0; j < units[u].njobs; ++j) {
      IpaJob& jb = *units[u].jobs[j];
      Transcript& tr = *units[u].tr;
      tr.absorb_pt(jb.label, &jb.P, 1, Fb);
      tr.absorb_fe(jb.label, &jb.v, 1, F);
      tr.challenge(jb.label, F, jb.q_raw);
      jb.nj = jb.n;
      jb.out->L.clear(); jb.out->R.clear();
    }
  auto active = [&](int u) { for (int j = 0; j < units[u].njobs; ++j) if (units[u].jobs[j]->nj > IPA_STOP) return true; return false; };
  int last = -1;                                                       // the unit enqueued last in this round
  auto enqueue = [&](int u) -> int {                                   // this round's L and R of the unit's active openings
    IpaUnit& un = units[u];
    vdf_ctx* ctx = un.ctx;
    size_t off[4] = {0, 0, 0, 0}, len[4];
    const vdf_fe* sc[4];
    int na = 0;
    for (int j = 0; j < un.njobs; ++j) {
      IpaJob& jb = *un.jobs[j];
      if (jb.nj <= IPA_STOP) continue;
      const vdf_fe* ab[2] = {(const vdf_fe*)jb.d_a, (const vdf_fe*)jb.d_b};
      HIPCALL(ctx, vdf_reduce(ctx, sd.field, VDF_REDUCE_IPA_CROSS, ab, nullptr, jb.nj, (vdf_fe*)jb.cross));      // pinned: no wait here
      HIPCALL(ctx, vdf_ipa_scalars(ctx, sd.field, (const vdf_fe*)jb.d_a, (const vdf_fe*)jb.d_s, jb.n, jb.nj, (vdf_fe*)jb.d_sL,
                                   (vdf_fe*)jb.d_sR));
      sc[2 * na] = (const vdf_fe*)jb.d_sL; sc[2 * na + 1] = (const vdf_fe*)jb.d_sR;
      len[2 * na] = len[2 * na + 1] = jb.n;
      ++na;
    }
    if (last >= 0 && units[last].ctx != ctx) HIPCALL(ctx, vdf_ctx_gate_accumulate(ctx, units[last].ctx, units[last].slot));
    HIPCALL(ctx, vdf_msm_batch(ctx, pp->gens, 2 * na, off, sc, len, 1, un.h_lr));
    HIPCALL(ctx, vdf_ctx_mark(ctx, un.slot));
    last = u;
    return VDF_OK;
  };
  auto finish = [&](int u) -> int {                                    // the round's points, challenges and folds of the unit
    IpaUnit& un = units[u];
    vdf_ctx* ctx = un.ctx;
    HIPCALL(ctx, vdf_ctx_sync_mark(ctx, un.slot));
    int a = 0;
    for (int j = 0; j < un.njobs; ++j) {
      IpaJob& jb = *un.jobs[j];
      if (jb.nj <= IPA_STOP) continue;
      Aff l0, r0;
      jac_to_aff2(un.h_lr[2 * a], un.h_lr[2 * a + 1], Fb, &l0, &r0);
      ++a;
      const Aff Lp = pt_to_aff(pt_add(pt_from_aff(l0, Fb), jb.Qtab->mul(jb.cross[0], F), Fb), Fb);
      const Aff Rp = pt_to_aff(pt_add(pt_from_aff(r0, Fb), jb.Qtab->mul(jb.cross[1], F), Fb), Fb);
      const Aff lr[2] = {Lp, Rp};
      un.tr->absorb_pt(jb.label, lr, 2, Fb);
      const Fe x = un.tr->challenge(jb.label, F, raw);
      const Fe xi = inverse(x, F);
      vdf_fe* vecs[2] = {(vdf_fe*)jb.d_a, (vdf_fe*)jb.d_b};
      const Fe c_lo[2] = {x, xi}, c_hi[2] = {xi, x};
      HIPCALL(ctx, vdf_fold_halves(ctx, sd.field, 2, vecs, (const vdf_fe*)c_lo, (const vdf_fe*)c_hi, jb.nj));
      HIPCALL(ctx, vdf_scale_pattern(ctx, sd.field, (vdf_fe*)jb.d_s, jb.n, jb.nj, (const vdf_fe*)&xi, (const vdf_fe*)&x));
      jb.out->L.push_back(Lp); jb.out->R.push_back(Rp);
      jb.nj >>= 1;
    }
    return VDF_OK;
  };
  for (int u = 0; u < nunits; ++u)
    if (active(u)) { int rc = enqueue(u); if (rc != VDF_OK) return rc; }
  for (int u = 0; u < nunits; ++u)                                     // Q and its table: under the first round's MSMs
    for (int j = 0; j < units[u].njobs; ++j) units[u].jobs[j]->make_q(pp->gen_u, Fb);
  for (;;) {
    std::vector<char> act(nunits);                                     // active in THIS round
    bool any = false;
    for (int u = 0; u < nunits; ++u) any |= (act[u] = active(u));
    if (!any) break;
    last = -1;
    for (int u = 0; u < nunits; ++u) {
      if (!act[u]) continue;
      { int rc = finish(u); if (rc != VDF_OK) return rc; }
      if (active(u)) { int rc = enqueue(u); if (rc != VDF_OK) return rc; }
    }
  }
  for (vdf_ctx* c : queues) HIPCALL(c, vdf_ctx_sync(c));
  for (int u = 0; u < nunits; ++u)
    for (int j = 0; j < units[u].njobs; ++j) {
      IpaJob& jb = *units[u].jobs[j];
      jb.out->a.resize(jb.nj);
      HIPCALL(sd.ctx, vdf_dev_memcpy(sd.ctx, jb.out->a.data(), jb.d_a, jb.nj * 32));
    }
  return VDF_OK;
}

// b is eq(rb, .): its fold is a closed form; the coefficient vector of the folded generators is a tensor-product table
struct IpaCheck {
  const char* label;
  size_t n;
  const std::vector<Fe>* rb;       // one entry per variable of the full vector
  Fe v;
  Aff P;
  const Ipa* proof;
  // state
  size_t k = 0, m = 0, idx = 0;
  int log_m = 0;
  Fe bfin;
};

// The transcript order of ipa_prove_units, up to the last check of each opening (sizes, challenges, b's fold, ab).  *ok =
// false for a proof that fails a size check or draws a zero challenge.
int ipa_replay(const Side& sd, Transcript& tr, IpaCheck* jobs, int njobs, IpaDeferred* out, bool* ok) {
  const Field& F = *sd.F;
  const Field& Fb = *sd.Fb;
  *ok = false;
  uint64_t raw[4];
  for (int q = 0; q < njobs; ++q) {
    IpaCheck& c = jobs[q];
    c.k = c.proof->L.size();
    c.m = ipa_final(c.n);
    int log_n = 0;
    while (((size_t)1 << c.log_m) < c.m) ++c.log_m;
    while (((size_t)1 << log_n) < c.n) ++log_n;
    if (((size_t)1 << log_n) != c.n || c.k != ipa_rounds(c.n) || c.proof->R.size() != c.k || c.proof->a.size() != c.m ||
        c.rb->size() != (size_t)log_n)
      return VDF_OK;
  }
  for (int q = 0; q < njobs; ++q) {
    IpaCheck& c = jobs[q];
    IpaDeferred& d = out[q];
    tr.absorb_pt(c.label, &c.P, 1, Fb);
    tr.absorb_fe(c.label, &c.v, 1, F);
    tr.challenge(c.label, F, d.q_raw);
    c.bfin = one(F);
    d.n = c.n; d.k = (int)c.k; d.log_m = c.log_m; d.P = c.P; d.v = c.v; d.a = c.proof->a;
    d.xs.resize(c.k); d.xis.resize(c.k);
  }
  for (;;) {
    bool any = false;
    for (int q = 0; q < njobs; ++q) {
      IpaCheck& c = jobs[q];
      IpaDeferred& d = out[q];
      if (c.idx >= c.k) continue;
      any = true;
      const size_t j = c.idx++;
      const Aff lr[2] = {c.proof->L[j], c.proof->R[j]};
      tr.absorb_pt(c.label, lr, 2, Fb);
      const Fe x = tr.challenge(c.label, F, raw);
      if (x.is_zero()) return VDF_OK;
      const Fe xi = inverse(x, F);
      const Fe& r = (*c.rb)[j];
      c.bfin = mul(c.bfin, add(mul(sub(one(F), r, F), xi, F), mul(r, x, F), F), F);
      d.xs[j] = x; d.xis[j] = xi;
    }
    if (!any) break;
  }
  for (int q = 0; q < njobs; ++q) {
    IpaCheck& c = jobs[q];
    IpaDeferred& d = out[q];
    d.lr_pts.resize(2 * c.k); d.lr_sc.resize(2 * c.k);
    for (size_t j = 0; j < c.k; ++j) {
      d.lr_pts[2 * j] = c.proof->L[j]; d.lr_sc[2 * j] = sqr(d.xs[j], F);
      d.lr_pts[2 * j + 1] = c.proof->R[j]; d.lr_sc[2 * j + 1] = sqr(d.xis[j], F);
    }
    // b folded in closed form: bfin (the rounds) times eq over the remaining variables
    Fe ab = zero();
    for (size_t i = 0; i < c.m; ++i) {
      Fe bi = c.bfin;
      for (int j = 0; j < c.log_m; ++j) {
        const Fe& r = (*c.rb)[c.k + j];
        bi = mul(bi, ((i >> (c.log_m - 1 - j)) & 1) ? r : sub(one(F), r, F), F);
      }
      ab = add(ab, mul(c.proof->a[i], bi, F), F);
    }
    d.ab = ab;
  }
  *ok = true;
  return VDF_OK;
}

}  // namespace
namespace vdfnova {
// One opening's check on its own: two device MSMs, sum_j x_j^2 L_j + x_j^-2 R_j (2k multiplications by full-size scalars: on
// the host they were the whole cost of verification, 0.25 ms each) and the folded generators against the sent vector.
// d_s: n device elements of scratch.
int ipa_check_one(const Side& sd, const IpaDeferred& d, void* d_s, bool* ok) {
  const Side* pp = &sd;
  vdf_ctx* ctx = sd.ctx;
  const Field& F = *sd.F;
  const Field& Fb = *sd.Fb;
  *ok = false;
  const Pt Qp = pt_mul(pt_from_aff(pp->gen_u, Fb), d.q_raw, 128, Fb);
  Pt acc = pt_add(pt_from_aff(d.P, Fb), pt_mul_fe(Qp, d.v, F, Fb), Fb);
  if (d.k) {
    vdf_bases* lrb = nullptr;
    HIPCALL(ctx, vdf_bases_upload(ctx, sd.curve, (const vdf_affine*)d.lr_pts.data(), 2 * d.k, &lrb));
    vdf_jac jlr;
    const int rc = vdf_msm(ctx, lrb, 0, (const vdf_fe*)d.lr_sc.data(), 2 * d.k, 1, &jlr);
    const std::string err = rc == VDF_OK ? "" : vdf_last_error(ctx);
    vdf_bases_free(lrb);
    if (rc != VDF_OK) return fail(rc, "vdf_msm (L, R): " + err);
    HIPCALL(ctx, vdf_ctx_sync(ctx));
    acc = pt_add(acc, pt_from_aff(jac_to_aff(jlr, Fb), Fb), Fb);
  }
  // coefficients of the original generators in sum_i a_i G'_i, G'_i the folded generators: the table of the performed
  // rounds over the top index bits times the sent vector over the low ones
  HIPCALL(ctx, vdf_pair_table_pattern(ctx, sd.field, (const vdf_fe*)d.xis.data(), (const vdf_fe*)d.xs.data(), d.k,
                                      (const vdf_fe*)d.a.data(), d.log_m, (vdf_fe*)d_s));
  vdf_jac jg;
  HIPCALL(ctx, vdf_msm(ctx, pp->gens, 0, (const vdf_fe*)d_s, d.n, 1, &jg));
  HIPCALL(ctx, vdf_ctx_sync(ctx));
  const Pt rhs = pt_add(pt_from_aff(jac_to_aff(jg, Fb), Fb), pt_mul_fe(Qp, d.ab, F, Fb), Fb);
  const Aff a1 = pt_to_aff(acc, Fb), a2 = pt_to_aff(rhs, Fb);
  *ok = memcmp(&a1, &a2, sizeof(Aff)) == 0;
  return VDF_OK;
}
}  // namespace vdfnova
namespace {

// tables of this many entries and fewer finish their sum-check on the host (a power of two; at least 2)
constexpr size_t SUMCHECK_HOST_TAIL = 512;
// the HBM spartan_m_check leaves free beside its tables (the rule of vdf_nova_compress_batch's groups: COMPRESS_HBM_RESERVE)
constexpr size_t VERIFY_HBM_RESERVE = (size_t)2 << 30;

// The passes of K proofs' rounds: one launch for all of them (vdf_*_batch), or the single call for one proof (the launches
// of vdf_nova_compress stay what they were)
int reduce_k(const Side& sd, int kind, size_t K, const vdf_fe* const* tabs, const Fe* u, size_t n, Fe* out) {
  vdf_ctx* ctx = sd.ctx;
  if (K == 1) HIPCALL(ctx, vdf_reduce(ctx, sd.field, kind, tabs, (const vdf_fe*)u, n, (vdf_fe*)out));
  else HIPCALL(ctx, vdf_reduce_batch(ctx, sd.field, kind, K, tabs, (const vdf_fe*)u, n, (vdf_fe*)out));
  return VDF_OK;
}
int fold_k(const Side& sd, int k, vdf_fe* const* vecs, const Fe* c_lo, const Fe* c_hi, size_t n) {
  vdf_ctx* ctx = sd.ctx;
  if (k <= 8) HIPCALL(ctx, vdf_fold_halves(ctx, sd.field, k, vecs, (const vdf_fe*)c_lo, (const vdf_fe*)c_hi, n));
  else HIPCALL(ctx, vdf_fold_halves_batch(ctx, sd.field, k, vecs, (const vdf_fe*)c_lo, (const vdf_fe*)c_hi, n));
  return VDF_OK;
}

// the scratch vectors of one proof's argument, in elements
size_t spartan_scratch_elems(const Side& sd) {
  const Layout L = layout_of(sd);
  return 5 * L.M + 2 * L.Z + 4 * L.NW + sd.ncols;
}

// K arguments on one side in lockstep: every round of every sum-check is one reduction and one fold for all K proofs, the
// M-vectors one transposed product, the openings' rounds ipa_prove_units.  Each proof keeps its own transcript, in the order
// of the single prover (spartan.py prove): only launches are shared, so every proof's bytes are those it has alone.
// arena: the block the scratch comes from (K x spartan_scratch_elems), or none.
int spartan_prove_many(const Side& sd, size_t K, const ProveIn* in, Arena* arena) {
  const Side* pp = &sd;
  vdf_ctx* ctx = sd.ctx;
  const Field& F = *sd.F;
  const Layout L = layout_of(sd);
  if (L.l1 > 24 || L.s > 24) return fail(VDF_ERR_BAD_LENGTH, "shape too large for the compression SNARK (2^24 entries)");
  if (L.NW > pp->num_gens) return fail(VDF_ERR_BAD_LENGTH, "not enough generators");
  const size_t nv = pp->num_vars, nc = pp->num_cons;
  struct Bufs { void *eq, *az, *bz, *cz, *e, *cols, *mvec, *zpad, *w, *s, *sL, *sR; };
  std::vector<Bufs> b(K);
  DevBufs bufs(ctx, arena);
  { int rc = bufs.reserve(K * spartan_scratch_elems(sd)); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
  for (size_t q = 0; q < K; ++q) {
    Bufs& x = b[q];
    for (void** p : {&x.eq, &x.az, &x.bz, &x.cz, &x.e}) { int rc = bufs.zeros(L.M, p); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    for (void** p : {&x.mvec, &x.zpad}) { int rc = bufs.zeros(L.Z, p); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    for (void** p : {&x.w, &x.s, &x.sL, &x.sR}) { int rc = bufs.zeros(L.NW, p); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    { int rc = bufs.zeros(pp->ncols, &x.cols); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
  }
  // pinned: per proof four result points of a round's batched MSM, then 2 x 2 cross terms
  const size_t per_pinned = 4 * sizeof(vdf_jac) + 4 * sizeof(Fe);
  char* h_pin = nullptr;
  HIPCALL(ctx, vdf_host_alloc(ctx, K * per_pinned, (void**)&h_pin));
  struct HostFree { vdf_ctx* c; void* p; ~HostFree() { vdf_host_free(c, p); } } hf{ctx, h_pin};

  std::vector<Transcript> tr(K, Transcript("compress"));
  std::vector<std::vector<Fe>> rx(K), ry(K);
  uint64_t raw[4];
  for (size_t q = 0; q < K; ++q) {
    const ProveIn& p = in[q];
    instance_bytes(tr[q], sd, p.cW, p.cE, p.u, p.X);
    HIPCALL(ctx, vdf_spmv3(ctx, pp->shape, (const vdf_fe*)p.d_z, (vdf_fe*)b[q].az, (vdf_fe*)b[q].bz, (vdf_fe*)b[q].cz));
    HIPCALL(ctx, vdf_dev_memcpy(ctx, b[q].e, p.d_E, nc * 32));
    std::vector<Fe> tau(L.s);
    for (int j = 0; j < L.s; ++j) tau[j] = tr[q].challenge("tau", F, raw);
    { int rc = eq_table_dev(sd, tau, b[q].eq); if (rc != VDF_OK) return rc; }
    p.out->outer.clear();
    p.out->inner.clear();
  }
  // ---- outer sum-check -----------------------------------------------------------------------------------
  {
    std::vector<const vdf_fe*> tabs(5 * K);
    std::vector<vdf_fe*> vecs(5 * K);
    std::vector<Fe> us(K), c_lo(5 * K), c_hi(5 * K);
    for (size_t q = 0; q < K; ++q) {
      void* t[5] = {b[q].eq, b[q].az, b[q].bz, b[q].cz, b[q].e};
      for (int k = 0; k < 5; ++k) { tabs[5 * q + k] = (const vdf_fe*)t[k]; vecs[5 * q + k] = (vdf_fe*)t[k]; }
      us[q] = in[q].u;
    }
    std::vector<std::array<Fe, 3>> ev(K);
    size_t n = L.M;
    for (; n > SUMCHECK_HOST_TAIL; n >>= 1) {
      { int rc = reduce_k(sd, VDF_REDUCE_R1CS_ROUND, K, tabs.data(), us.data(), n, ev[0].data()); if (rc != VDF_OK) return rc; }
      for (size_t q = 0; q < K; ++q) {
        tr[q].absorb_fe("outer", ev[q].data(), 3, F);
        const Fe r = tr[q].challenge("outer", F, raw);
        const Fe omr = sub(one(F), r, F);
        for (int k = 0; k < 5; ++k) { c_lo[5 * q + k] = omr; c_hi[5 * q + k] = r; }
        in[q].out->outer.push_back(ev[q]);
        rx[q].push_back(r);
      }
      { int rc = fold_k(sd, (int)(5 * K), vecs.data(), c_lo.data(), c_hi.data(), n); if (rc != VDF_OK) return rc; }
    }
    // The last rounds on the HOST: a round over a table of a few hundred entries is two launches, a synchronisation and the
    // transcript -- ~0.25 ms of latency for microseconds of arithmetic -- nine times per sum-check.  The tables come down once
    // (5 x 512 elements) and the same sums, the same challenges and the same folds follow in host arithmetic (exact: the
    // values are the kernels', snark.hip reduce_term<2> / k_fold_halves).
    HIPCALL(ctx, vdf_ctx_sync(ctx));
    for (size_t q = 0; q < K; ++q) {
      const Fe u = in[q].u;
      std::vector<Fe> hv[5];
      for (int k = 0; k < 5; ++k) { hv[k].resize(n); HIPCALL(ctx, vdf_dev_memcpy(ctx, hv[k].data(), vecs[5 * q + k], n * 32)); }
      for (size_t m = n; m > 1; m >>= 1) {
        const size_t h = m / 2;
        std::array<Fe, 3> e = {zero(), zero(), zero()};
        for (size_t i = 0; i < h; ++i) {
          Fe lo[5], d[5], v[5];
          for (int k = 0; k < 5; ++k) { lo[k] = hv[k][i]; d[k] = sub(hv[k][h + i], lo[k], F); }
          auto term = [&](const Fe* w) { return mul(w[0], sub(sub(mul(w[1], w[2], F), mul(u, w[3], F), F), w[4], F), F); };
          e[0] = add(e[0], term(lo), F);
          for (int k = 0; k < 5; ++k) v[k] = add(lo[k], add(d[k], d[k], F), F);
          e[1] = add(e[1], term(v), F);
          for (int k = 0; k < 5; ++k) v[k] = add(v[k], d[k], F);
          e[2] = add(e[2], term(v), F);
        }
        tr[q].absorb_fe("outer", e.data(), 3, F);
        const Fe r = tr[q].challenge("outer", F, raw);
        const Fe omr = sub(one(F), r, F);
        for (int k = 0; k < 5; ++k)
          for (size_t i = 0; i < h; ++i) hv[k][i] = add(mul(omr, hv[k][i], F), mul(r, hv[k][h + i], F), F);
        in[q].out->outer.push_back(e);
        rx[q].push_back(r);
      }
      Spartan* o = in[q].out;
      o->claims[0] = hv[1][0]; o->claims[1] = hv[2][0]; o->claims[2] = hv[3][0]; o->claims[3] = hv[4][0];
    }
  }
  std::vector<Fe> rho(K);
  for (size_t q = 0; q < K; ++q) {
    tr[q].absorb_fe("claims", in[q].out->claims, 4, F);
    rho[q] = tr[q].challenge("rho", F, raw);
  }
  // ---- inner sum-check -----------------------------------------------------------------------------------
  // the outer tables are spent: az holds eq(r_x, .)
  for (size_t q = 0; q < K; ++q) { int rc = eq_table_dev(sd, rx[q], b[q].az); if (rc != VDF_OK) return rc; }
  if (K == 1) {
    int rc = m_vector_dev(sd, L, b[0].az, rho[0], b[0].cols, b[0].mvec);
    if (rc != VDF_OK) return rc;
  } else {
    std::vector<const vdf_fe*> eqs(K);
    std::vector<vdf_fe*> cols(K);
    for (size_t q = 0; q < K; ++q) { eqs[q] = (const vdf_fe*)b[q].az; cols[q] = (vdf_fe*)b[q].cols; }
    HIPCALL(ctx, vdf_spmv3_t_batch(ctx, pp->shape, K, eqs.data(), (const vdf_fe*)rho.data(), cols.data()));
    for (size_t q = 0; q < K; ++q) {                           // M(y) in the padded layout (m_vector_dev)
      HIPCALL(ctx, vdf_dev_memset(ctx, b[q].mvec, 0, L.Z * 32));
      HIPCALL(ctx, vdf_dev_memcpy(ctx, b[q].mvec, b[q].cols, nv * 32));
      HIPCALL(ctx, vdf_dev_memcpy(ctx, (char*)b[q].mvec + L.NW * 32, (const char*)b[q].cols + nv * 32, (1 + NUM_IO) * 32));
    }
  }
  for (size_t q = 0; q < K; ++q) {
    HIPCALL(ctx, vdf_dev_memcpy(ctx, b[q].zpad, in[q].d_z, nv * 32));
    HIPCALL(ctx, vdf_dev_memcpy(ctx, (char*)b[q].zpad + L.NW * 32, (const char*)in[q].d_z + nv * 32, (1 + NUM_IO) * 32));
    HIPCALL(ctx, vdf_dev_memcpy(ctx, b[q].w, in[q].d_z, nv * 32));
  }
  {
    std::vector<const vdf_fe*> tabs(2 * K);
    std::vector<vdf_fe*> vecs(2 * K);
    std::vector<Fe> c_lo(2 * K), c_hi(2 * K);
    for (size_t q = 0; q < K; ++q) {
      tabs[2 * q] = (const vdf_fe*)b[q].mvec; tabs[2 * q + 1] = (const vdf_fe*)b[q].zpad;
      vecs[2 * q] = (vdf_fe*)b[q].mvec; vecs[2 * q + 1] = (vdf_fe*)b[q].zpad;
    }
    std::vector<std::array<Fe, 2>> ev(K);
    size_t n = L.Z;
    for (; n > SUMCHECK_HOST_TAIL; n >>= 1) {
      { int rc = reduce_k(sd, VDF_REDUCE_QUADRATIC_ROUND, K, tabs.data(), nullptr, n, ev[0].data()); if (rc != VDF_OK) return rc; }
      for (size_t q = 0; q < K; ++q) {
        tr[q].absorb_fe("inner", ev[q].data(), 2, F);
        const Fe r = tr[q].challenge("inner", F, raw);
        const Fe omr = sub(one(F), r, F);
        c_lo[2 * q] = c_lo[2 * q + 1] = omr; c_hi[2 * q] = c_hi[2 * q + 1] = r;
        in[q].out->inner.push_back(ev[q]);
        ry[q].push_back(r);
      }
      { int rc = fold_k(sd, (int)(2 * K), vecs.data(), c_lo.data(), c_hi.data(), n); if (rc != VDF_OK) return rc; }
    }
    HIPCALL(ctx, vdf_ctx_sync(ctx));                            // the last rounds on the host (as in the outer sum-check)
    for (size_t q = 0; q < K; ++q) {
      std::vector<Fe> hv[2];
      for (int k = 0; k < 2; ++k) { hv[k].resize(n); HIPCALL(ctx, vdf_dev_memcpy(ctx, hv[k].data(), vecs[2 * q + k], n * 32)); }
      for (size_t m = n; m > 1; m >>= 1) {
        const size_t h = m / 2;
        std::array<Fe, 2> e = {zero(), zero()};
        for (size_t i = 0; i < h; ++i) {
          const Fe p0 = hv[0][i], p1 = hv[0][h + i], q0 = hv[1][i], q1 = hv[1][h + i];
          e[0] = add(e[0], mul(p0, q0, F), F);
          e[1] = add(e[1], mul(sub(add(p1, p1, F), p0, F), sub(add(q1, q1, F), q0, F), F), F);
        }
        tr[q].absorb_fe("inner", e.data(), 2, F);
        const Fe r = tr[q].challenge("inner", F, raw);
        const Fe omr = sub(one(F), r, F);
        for (int k = 0; k < 2; ++k)
          for (size_t i = 0; i < h; ++i) hv[k][i] = add(mul(omr, hv[k][i], F), mul(r, hv[k][h + i], F), F);
        in[q].out->inner.push_back(e);
        ry[q].push_back(r);
      }
    }
  }
  // ---- openings ----------------------------------------------------------------------------------------------
  // mvec is spent: reuse it for eq(r_y[1:], .) (NW entries)
  for (size_t q = 0; q < K; ++q) {
    std::vector<Fe> rest(ry[q].begin() + 1, ry[q].end());
    int rc = eq_table_dev(sd, rest, b[q].mvec);
    if (rc != VDF_OK) return rc;
  }
  {
    std::vector<const vdf_fe*> tabs(2 * K);
    for (size_t q = 0; q < K; ++q) { tabs[2 * q] = (const vdf_fe*)b[q].w; tabs[2 * q + 1] = (const vdf_fe*)b[q].mvec; }
    std::vector<Fe> we(K);
    { int rc = reduce_k(sd, VDF_REDUCE_DOT, K, tabs.data(), nullptr, L.NW, we.data()); if (rc != VDF_OK) return rc; }
    for (size_t q = 0; q < K; ++q) {
      in[q].out->w_eval = we[q];
      tr[q].absorb_fe("weval", &in[q].out->w_eval, 1, F);
    }
  }
  // the two openings of a proof: W: a = W padded, b = eq(r_y[1:], .); E: a = E padded to M (fresh copy: e was folded by the
  // sum-check), b = eq(r_x, .).  Each needs its own coefficient and scalar vectors: the E opening's live in buffers the
  // sum-checks are done with (eq, bz, cz: M entries each; az holds eq(r_x, .)).
  std::vector<Fe> ones_lo(24, one(F));
  std::vector<IpaJob> jobs(2 * K);
  for (size_t q = 0; q < K; ++q) {
    Bufs& x = b[q];
    HIPCALL(ctx, vdf_pair_table(ctx, sd.field, (const vdf_fe*)ones_lo.data(), (const vdf_fe*)ones_lo.data(), L.l1 - 1, (vdf_fe*)x.s));
    HIPCALL(ctx, vdf_dev_memset(ctx, x.e, 0, L.M * 32));
    HIPCALL(ctx, vdf_dev_memcpy(ctx, x.e, in[q].d_E, nc * 32));
    HIPCALL(ctx, vdf_pair_table(ctx, sd.field, (const vdf_fe*)ones_lo.data(), (const vdf_fe*)ones_lo.data(), L.s, (vdf_fe*)x.eq));
    Fe* h_cross = reinterpret_cast<Fe*>(h_pin + q * per_pinned + 4 * sizeof(vdf_jac));
    IpaJob& w = jobs[2 * q];
    IpaJob& e = jobs[2 * q + 1];
    w.label = "ipaW"; w.n = L.NW; w.d_a = x.w; w.d_b = x.mvec; w.d_s = x.s; w.d_sL = x.sL; w.d_sR = x.sR;
    w.v = in[q].out->w_eval; w.P = in[q].cW; w.out = &in[q].out->ipaW; w.cross = h_cross;
    e.label = "ipaE"; e.n = L.M; e.d_a = x.e; e.d_b = x.az; e.d_s = x.eq; e.d_sL = x.bz; e.d_sR = x.cz;
    e.v = in[q].out->claims[3]; e.P = in[q].cE; e.out = &in[q].out->ipaE; e.cross = h_cross + 2;
  }
  std::vector<IpaUnit> units;
  vdf_jac* h_lr0 = reinterpret_cast<vdf_jac*>(h_pin);
  if (K == 1 && sd.ctx_b) {                                   // one proof, two queues: each opening a unit of its own
    units.push_back({&tr[0], {&jobs[0], nullptr}, 1, ctx, IPA_MARK, h_lr0});
    units.push_back({&tr[0], {&jobs[1], nullptr}, 1, sd.ctx_b, IPA_MARK, h_lr0 + 2});
  } else {                                                    // a unit per proof, round robin over the side's queues
    vdf_ctx* qs[2] = {ctx, sd.ctx_b};
    const size_t nq = sd.ctx_b ? 2 : 1;
    if ((K + nq - 1) / nq > (size_t)IPA_UNITS_PER_QUEUE) return fail(VDF_ERR_BAD_ARG, "too many proofs in one lockstep group");
    for (size_t q = 0; q < K; ++q)
      units.push_back({&tr[q], {&jobs[2 * q], &jobs[2 * q + 1]}, 2, qs[q % nq], IPA_MARK + (int)(q / nq),
                       reinterpret_cast<vdf_jac*>(h_pin + q * per_pinned)});
  }
  return ipa_prove_units(sd, units.data(), (int)units.size());
}


// What is left of the inner sum-check once the transcript is replayed: claim == M(r_x, r_y) z(r_y), with M(r_x, r_y) the one
// value the verifier needs the device for.  The transcript does not absorb it and nothing after it depends on it, so the
// comparison can wait until every proof of a batch has been replayed (spartan_m_check).
struct MDeferred {
  std::vector<Fe> rx, ry;
  Fe rho, claim, z_ry;
};

// The verifier's transcript replay of one side's argument on the host alone, without a device call or wait: sizes, both
// sum-checks up to the last comparison of the inner one (left in *md), the openings up to their deferred group checks
// (out[0]: W, out[1]: E).  *ok = false when an exact check fails.
int spartan_replay_host(const Side& sd, const Aff& cW, const Aff& cE, const Fe& u, const Fe* X, const Spartan& pf, IpaDeferred out[2],
                        MDeferred* md, bool* ok) {
  const Field& F = *sd.F;
  const Layout L = layout_of(sd);
  *ok = false;
  if ((int)pf.outer.size() != L.s || (int)pf.inner.size() != L.l1) return VDF_OK;
  Transcript tr("compress");
  instance_bytes(tr, sd, cW, cE, u, X);
  uint64_t raw[4];
  std::vector<Fe> tau(L.s);
  std::vector<Fe>& rx = md->rx;
  std::vector<Fe>& ry = md->ry;
  rx.clear(); ry.clear();
  for (int j = 0; j < L.s; ++j) tau[j] = tr.challenge("tau", F, raw);
  // outer
  Fe claim = zero();
  for (const auto& ev : pf.outer) {
    const Fe y[4] = {ev[0], sub(claim, ev[0], F), ev[1], ev[2]};
    tr.absorb_fe("outer", ev.data(), 3, F);
    const Fe r = tr.challenge("outer", F, raw);
    claim = interpolate(y, 4, r, F);
    rx.push_back(r);
  }
  Fe eq_tau = one(F);
  for (int j = 0; j < L.s; ++j)
    eq_tau = mul(eq_tau, add(mul(tau[j], rx[j], F), mul(sub(one(F), tau[j], F), sub(one(F), rx[j], F), F), F), F);
  const Fe a = pf.claims[0], b = pf.claims[1], c = pf.claims[2], e = pf.claims[3];
  if (claim != mul(eq_tau, sub(sub(mul(a, b, F), mul(u, c, F), F), e, F), F)) return VDF_OK;
  tr.absorb_fe("claims", pf.claims, 4, F);
  const Fe rho = tr.challenge("rho", F, raw);
  // inner
  claim = add(a, add(mul(rho, b, F), mul(sqr(rho, F), c, F), F), F);
  for (const auto& ev : pf.inner) {
    const Fe y[3] = {ev[0], sub(claim, ev[0], F), ev[1]};
    tr.absorb_fe("inner", ev.data(), 2, F);
    const Fe r = tr.challenge("inner", F, raw);
    claim = interpolate(y, 3, r, F);
    ry.push_back(r);
  }
  // z(r_y) = (1 - r_y[0]) W~(rest) + r_y[0] * (u, X)~(rest); index i of the public half has bits MSB-first over rest
  std::vector<Fe> rest(ry.begin() + 1, ry.end());
  const int k = (int)rest.size();
  Fe pub = zero();
  for (int i = 0; i < 1 + NUM_IO; ++i) {
    Fe w = one(F);
    for (int j = 0; j < k; ++j) w = mul(w, ((i >> (k - 1 - j)) & 1) ? rest[j] : sub(one(F), rest[j], F), F);
    pub = add(pub, mul(w, i == 0 ? u : X[i - 1], F), F);
  }
  md->rho = rho;
  md->claim = claim;
  md->z_ry = add(mul(sub(one(F), ry[0], F), pf.w_eval, F), mul(ry[0], pub, F), F);
  tr.absorb_fe("weval", &pf.w_eval, 1, F);
  IpaCheck checks[2];
  checks[0].label = "ipaW"; checks[0].n = L.NW; checks[0].rb = &rest; checks[0].v = pf.w_eval; checks[0].P = cW; checks[0].proof = &pf.ipaW;
  checks[1].label = "ipaE"; checks[1].n = L.M; checks[1].rb = &rx; checks[1].v = e; checks[1].P = cE; checks[1].proof = &pf.ipaE;
  return ipa_replay(sd, tr, checks, 2, out, ok);
}

// One proof's deferred comparison by the single verifier's device sequence: eq(r_x, .) -> transposed product -> dot with
// eq(r_y, .), and a wait for the element.
int spartan_m_single(const Side& sd, const MDeferred& md, bool* ok) {
  const Side* pp = &sd;
  vdf_ctx* ctx = sd.ctx;
  const Field& F = *sd.F;
  const Layout L = layout_of(sd);
  *ok = false;
  DevBufs bufs(ctx, sd.arena);
  { int rc = bufs.reserve(L.M + pp->ncols + 2 * L.Z); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
  void *d_eq_rx, *d_cols, *d_mvec, *d_eq_ry;
  { int rc = bufs.zeros(L.M, &d_eq_rx); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
  { int rc = bufs.zeros(pp->ncols, &d_cols); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
  for (void** p : {&d_mvec, &d_eq_ry}) { int rc = bufs.zeros(L.Z, p); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
  { int rc = eq_table_dev(sd, md.rx, d_eq_rx); if (rc != VDF_OK) return rc; }
  { int rc = m_vector_dev(sd, L, d_eq_rx, md.rho, d_cols, d_mvec); if (rc != VDF_OK) return rc; }
  { int rc = eq_table_dev(sd, md.ry, d_eq_ry); if (rc != VDF_OK) return rc; }
  Fe m_ry;
  {
    const vdf_fe* tabs[2] = {(const vdf_fe*)d_mvec, (const vdf_fe*)d_eq_ry};
    HIPCALL(ctx, vdf_reduce(ctx, sd.field, VDF_REDUCE_DOT, tabs, nullptr, L.Z, (vdf_fe*)&m_ry));
  }
  *ok = md.claim == mul(m_ry, md.z_ry, F);
  return VDF_OK;
}

}  // namespace
namespace vdfnova {
// The single verifier's replay of one side: the host part, then M(r_x, r_y) on the device.
int spartan_replay(const Side& sd, const Aff& cW, const Aff& cE, const Fe& u, const Fe* X, const Spartan& pf, IpaDeferred out[2],
                   bool* ok) {
  MDeferred md;
  { int rc = spartan_replay_host(sd, cW, cE, u, X, pf, out, &md, ok); if (rc != VDF_OK || !*ok) return rc; }
  return spartan_m_single(sd, md, ok);
}
}  // namespace vdfnova
namespace {

// The deferred comparisons of n proofs of one side (vdf_nova_verify_compressed_batch): the n pairs of eq tables (asynchronous,
// no wait between them), then every M(r_x, r_y) of a group by ONE pass over the shape's rows (vdf_sparse_eval_multi, with the
// column map of the padded layout m_vector_dev builds by copies: W at [0, NW), u and X from NW), one wait per group.  A group
// is at most `width` points, and fewer when the free HBM (less the reserve vdf_nova_compress_batch keeps) does not hold the
// tables beside the side's block.  stats: launches, points evaluated, points whose comparison failed.
int spartan_m_check(const Side& sd, const MDeferred* const items[], size_t n, size_t width, bool ok[], uint64_t stats[3]) {
  vdf_ctx* ctx = sd.ctx;
  const Field& F = *sd.F;
  const Layout L = layout_of(sd);
  for (size_t q = 0; q < n; ++q) ok[q] = false;
  if (n == 0) return VDF_OK;
  const size_t per_point = 32 * (L.M + L.Z);
  width = std::max<size_t>(1, std::min<size_t>({width, n, (size_t)VDF_SPARSE_EVAL_MAX}));
  Arena* arena = sd.arena;
  if (arena->cap < width * per_point) {
    size_t free_b = 0, total_b = 0;
    HIPCALL(ctx, vdf_dev_mem_info(ctx, &free_b, &total_b));
    const size_t avail = arena->cap + (free_b > VERIFY_HBM_RESERVE ? free_b - VERIFY_HBM_RESERVE : 0);
    width = std::max<size_t>(1, std::min(width, avail / per_point));
    if (arena->cap < width * per_point) {
      if (arena->p) { vdf_ctx_sync(ctx); vdf_dev_free(ctx, arena->p); arena->p = nullptr; arena->cap = 0; }
      int rc = vdf_dev_alloc(ctx, width * per_point, &arena->p);
      if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx));
      arena->cap = width * per_point;
    }
  }
  std::vector<const vdf_fe*> ex(width), ey(width);
  std::vector<Fe> rho(width), m(width);
  for (size_t g0 = 0; g0 < n; g0 += width) {
    const size_t K = std::min(width, n - g0);
    for (size_t q = 0; q < K; ++q) {                                  // (a table is written whole: the block needs no memset)
      char* base = static_cast<char*>(arena->p) + q * per_point;
      const MDeferred& d = *items[g0 + q];
      { int rc = eq_table_dev(sd, d.rx, base); if (rc != VDF_OK) return rc; }
      { int rc = eq_table_dev(sd, d.ry, base + 32 * L.M); if (rc != VDF_OK) return rc; }
      ex[q] = (const vdf_fe*)base; ey[q] = (const vdf_fe*)(base + 32 * L.M);
      rho[q] = d.rho;
    }
    HIPCALL(ctx, vdf_sparse_eval_multi(ctx, sd.shape, (int)K, ex.data(), L.M, ey.data(), L.Z, (const vdf_fe*)rho.data(), sd.num_vars, L.NW,
                                       (vdf_fe*)m.data()));
    stats[0] += 1; stats[1] += K;
    for (size_t q = 0; q < K; ++q) {
      const MDeferred& d = *items[g0 + q];
      ok[g0 + q] = d.claim == mul(m[q], d.z_ry, F);
      if (!ok[g0 + q]) stats[2] += 1;
    }
  }
  return VDF_OK;
}

}  // namespace

namespace vdfnova {

// instance fold on the host: U + r u with the cross-term commitment T (two 128-bit scalar multiplications)
Inst fold_instance(const Side& sd, const Inst& U, const Inst& u, const Aff& T, const uint64_t r[4]) {
  const Field& F = *sd.F;
  const Field& Fb = *sd.Fb;
  const Fe rf = int_to_fe(r, F);
  Inst o;
  o.comm_W = pt_to_aff(pt_add(pt_from_aff(U.comm_W, Fb), pt_mul(pt_from_aff(u.comm_W, Fb), r, 128, Fb), Fb), Fb);
  o.comm_E = pt_to_aff(pt_add(pt_from_aff(U.comm_E, Fb), pt_mul(pt_from_aff(T, Fb), r, 128, Fb), Fb), Fb);
  o.u = add(U.u, rf, F);
  for (int k = 0; k < NUM_IO; ++k) o.X[k] = add(U.X[k], mul(rf, u.X[k], F), F);
  return o;
}

void fold_challenge(const vdf_pp* pp, const Inst& U2, const Inst& l2, const Aff& T2, uint64_t r[4]) {
  const Field& F2 = *pp->s[SECONDARY].F;
  uint64_t ux[2][4];
  for (int k = 0; k < 2; ++k) fe_to_int(l2.X[k], F2, ux[k]);
  hash_challenge(pp->s[PRIMARY].field, pp->params[PRIMARY], to_relaxed(U2, F2), l2.comm_W, ux, T2, r, pp->ro);
}

size_t spartan_flat_size(const Spartan& p) {
  return 32 * (3 * p.outer.size() + 4 + 2 * p.inner.size() + 1 + p.ipaW.a.size() + p.ipaE.a.size()) + 128 * (p.ipaW.L.size() + p.ipaE.L.size());
}
size_t spartan_wire_size(const Layout& L) {
  return 32 * (3 * (size_t)L.s + 4 + 2 * (size_t)L.l1 + 1 + ipa_final(L.NW) + ipa_final(L.M)) + 64 * (ipa_rounds(L.NW) + ipa_rounds(L.M));
}
void spartan_resize(Spartan& p, const Layout& L) {
  p.outer.resize(L.s); p.inner.resize(L.l1);
  p.ipaW.L.resize(ipa_rounds(L.NW)); p.ipaW.R.resize(ipa_rounds(L.NW)); p.ipaW.a.resize(ipa_final(L.NW));
  p.ipaE.L.resize(ipa_rounds(L.M)); p.ipaE.R.resize(ipa_rounds(L.M)); p.ipaE.a.resize(ipa_final(L.M));
}

// the statement part of a compressed proof on the wire: instances with 32-byte points, then both z_i
// without the primary z_i (32 bytes per element of the step circuit's arity)
constexpr size_t STATEMENT_WIRE_FIXED = 5 * 32 * 2 + 3 * 32 + 32 + 32;
size_t statement_wire(size_t arity) { return STATEMENT_WIRE_FIXED + 32 * arity; }

// vdf_nova_compress_batch: proofs per lockstep group, and the HBM left free beside the groups' scratch
constexpr size_t COMPRESS_LOCKSTEP = 8;
constexpr size_t COMPRESS_HBM_RESERVE = (size_t)2 << 30;

// The statement of a compressed proof, and the last secondary instance folded into the running one (NIFS, as a prove_step
// would) into scratch d_fz / d_fE: the proof keeps its instances; its secondary cross-term buffers (d_abc2, d_T) are
// overwritten.  *f2: the folded instance.
int compress_prelude(const vdf_proof* p, vdf_pp* pp, vdf_snark* s, void* d_fz, void* d_fE, Inst* f2) {
  vdf_ctx* ctx = pp->ctx;
  const Side& S2 = pp->s[SECONDARY];
  s->t = pp->t;
  s->field = pp->field;
  memcpy(s->digest, pp->digest, 32);
  s->r_U1 = p->r[PRIMARY].inst; s->r_U2 = p->r[SECONDARY].inst; s->l_u2 = p->l2;
  s->zi1 = p->zi[PRIMARY];
  s->zi2[0] = p->zi[SECONDARY][0];
  vdf_proof* q = const_cast<vdf_proof*>(p);
  SideState& s2 = q->r[SECONDARY];
  { int rc = cross_all(ctx, S2, s2, p->d_l2z); if (rc != VDF_OK) return rc; }
  vdf_jac jt;
  HIPCALL(ctx, vdf_msm(ctx, S2.gens, 0, (const vdf_fe*)s2.d_T, S2.num_cons, 1, &jt));
  s->T2 = jac_to_aff(jt, *S2.Fb);
  uint64_t r[4];
  fold_challenge(pp, s->r_U2, s->l_u2, s->T2, r);
  *f2 = fold_instance(S2, s->r_U2, s->l_u2, s->T2, r);
  const Fe rf = int_to_fe(r, *S2.F);
  HIPCALL(ctx, vdf_axpy(ctx, S2.field, (const vdf_fe*)s2.d_z, (const vdf_fe*)&rf, (const vdf_fe*)p->d_l2z, S2.ncols, (vdf_fe*)d_fz));
  HIPCALL(ctx, vdf_axpy(ctx, S2.field, (const vdf_fe*)s2.d_E, (const vdf_fe*)&rf, (const vdf_fe*)s2.d_T, S2.num_cons, (vdf_fe*)d_fE));
  return VDF_OK;
}

// the queues of the two sides' arguments (created on first use; the caller holds pp->aux_mu)
int compress_queues(vdf_pp* pp) {
  vdf_ctx* ctx = pp->ctx;
  if (!pp->aux_ctx) {
    const int dev = vdf_ctx_device(ctx);
    if (vdf_ctx_create_pooled(&dev, 1, VDF_QUEUE_SIDE, &pp->aux_ctx) != VDF_OK) return fail(VDF_ERR_DEVICE, std::string("compress: second context: ") + vdf_last_error(nullptr));
  }
  if (!pp->aux_ctx2 && pp->tune.compress_queues) {
    const int dev = vdf_ctx_device(ctx);
    if (vdf_ctx_create_pooled(&dev, 1, VDF_QUEUE_SIDE, &pp->aux_ctx2) != VDF_OK) return fail(VDF_ERR_DEVICE, std::string("compress: third context: ") + vdf_last_error(nullptr));
  }
  return VDF_OK;
}

// Both sides' arguments of K proofs: the two are independent (a transcript each), so the secondary side's runs on a second
// queue of the device, driven by a second host thread, beside the primary's -- its small latency-bound MSMs and its host
// work (transcript, point arithmetic between rounds) disappear under the primary side's 2^19-generator MSMs.
// (nova-snark's CompressedSNARK::prove runs the two provers in parallel as well.)  in1 / in2: K statements per side;
// arena1 / arena2: the sides' scratch blocks.
int prove_both_sides(vdf_pp* pp, size_t K, const ProveIn* in1, const ProveIn* in2, Arena* arena1, Arena* arena2) {
  vdf_ctx* ctx = pp->ctx;
  { int rc = compress_queues(pp); if (rc != VDF_OK) return rc; }
  vdf_ctx* cb = pp->aux_ctx;
  HIPCALL(cb, vdf_ctx_set_async(cb, 1));
  HIPCALL(cb, vdf_ctx_wait(cb, ctx));                                // the folded secondary witnesses were made on the first queue
  Side S2b = pp->s[SECONDARY];
  S2b.ctx = cb;
  int rc2 = VDF_OK;
  std::string err2;
  std::thread side2([&] {
    try { rc2 = spartan_prove_many(S2b, K, in2, arena2); }
    catch (const std::exception& ex) { rc2 = VDF_ERR_DEVICE; err2 = ex.what(); }
    if (rc2 != VDF_OK && err2.empty()) err2 = vdf_nova_last_error();  // (the message is per thread: carried over by hand)
    (void)vdf_ctx_sync(cb);
  });
  int rc = VDF_OK;
  Side S1b = pp->s[PRIMARY];
  S1b.ctx_b = pp->tune.compress_queues ? pp->aux_ctx2 : nullptr;   // the primary side's second queue
  try { rc = spartan_prove_many(S1b, K, in1, arena1); }
  catch (...) { side2.join(); throw; }
  side2.join();
  if (rc != VDF_OK) return rc;
  if (rc2 != VDF_OK) return fail(rc2, "compress, secondary side: " + err2);
  return VDF_OK;
}

// the arena of a lockstep group: freed with it (the parameter set keeps only the single prover's blocks)
struct OwnedArena : Arena {
  vdf_ctx* ctx;
  explicit OwnedArena(vdf_ctx* c) : ctx(c) {}
  ~OwnedArena() { if (p) vdf_dev_free(ctx, p); }
};
}  // namespace vdfnova

extern "C" {

int vdf_nova_compress(const vdf_proof* p, vdf_pp* pp, vdf_snark** out) {
  return nova_guard([&]() -> int {
    if (!p || !pp || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (p->pp != pp) return fail(VDF_ERR_BAD_ARG, "proof was made under other public parameters");
    if (p->i == 0) return fail(VDF_ERR_BAD_LENGTH, "nothing to compress");
    { int rc = finalize_l2(p); if (rc != VDF_OK) return rc; }
    vdf_ctx* ctx = pp->ctx;
    const Side& S2 = pp->s[SECONDARY];
    int was_async = 0;
    HIPCALL(ctx, vdf_ctx_get_async(ctx, &was_async));
    HIPCALL(ctx, vdf_ctx_sync(ctx));
    HIPCALL(ctx, vdf_ctx_set_async(ctx, 1));
    struct Restore { vdf_ctx* c; int a; ~Restore() { vdf_ctx_sync(c); vdf_ctx_set_async(c, a); } } restore{ctx, was_async};
    std::unique_ptr<vdf_snark> s(new vdf_snark());
    DevBufs bufs(ctx);
    void *d_fz, *d_fE;
    { int rc = bufs.zeros(S2.ncols, &d_fz); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    { int rc = bufs.zeros(S2.num_cons, &d_fE); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
    Inst f2;
    { int rc = compress_prelude(p, pp, s.get(), d_fz, d_fE, &f2); if (rc != VDF_OK) return rc; }
    std::lock_guard<std::mutex> aux_lock(pp->aux_mu);
    const ProveIn in1{s->r_U1.comm_W, s->r_U1.comm_E, s->r_U1.u, s->r_U1.X, p->r[PRIMARY].d_z, p->r[PRIMARY].d_E, &s->sp[0]};
    const ProveIn in2{f2.comm_W, f2.comm_E, f2.u, f2.X, d_fz, d_fE, &s->sp[1]};
    { int rc = prove_both_sides(pp, 1, &in1, &in2, &pp->arena[PRIMARY], &pp->arena[SECONDARY]); if (rc != VDF_OK) return rc; }
    *out = s.release();
    return VDF_OK;
  });
}

// Many proofs under one parameter set: groups of up to COMPRESS_LOCKSTEP distinct proofs move through both sides'
// arguments in lockstep (spartan_prove_many); a proof named more than once is compressed once and copied.
int vdf_nova_compress_batch(vdf_pp* pp, size_t count, const vdf_proof* const proofs[], vdf_snark* out[]) {
  return nova_guard([&]() -> int {
    if (!pp || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (count == 0) return VDF_OK;
    for (size_t q = 0; q < count; ++q) out[q] = nullptr;
    if (!proofs) return fail(VDF_ERR_BAD_ARG, "null argument");
    for (size_t q = 0; q < count; ++q) {
      const vdf_proof* p = proofs[q];
      if (!p) return fail(VDF_ERR_BAD_ARG, "entry " + std::to_string(q) + ": null proof");
      if (p->pp != pp) return fail(VDF_ERR_BAD_ARG, "entry " + std::to_string(q) + ": proof was made under other public parameters");
      if (p->i == 0) return fail(VDF_ERR_BAD_LENGTH, "entry " + std::to_string(q) + ": nothing to compress");
    }
    // distinct proofs in order of first appearance; slot q is a copy of the snark of uniq[which[q]]
    std::vector<const vdf_proof*> uniq;
    std::vector<size_t> which(count);
    for (size_t q = 0; q < count; ++q) {
      size_t k = 0;
      while (k < uniq.size() && uniq[k] != proofs[q]) ++k;
      if (k == uniq.size()) uniq.push_back(proofs[q]);
      which[q] = k;
    }
    for (const vdf_proof* p : uniq) { int rc = finalize_l2(p); if (rc != VDF_OK) return rc; }
    vdf_ctx* ctx = pp->ctx;
    const Side& S1 = pp->s[PRIMARY];
    const Side& S2 = pp->s[SECONDARY];
    int was_async = 0;
    HIPCALL(ctx, vdf_ctx_get_async(ctx, &was_async));
    HIPCALL(ctx, vdf_ctx_sync(ctx));
    HIPCALL(ctx, vdf_ctx_set_async(ctx, 1));
    struct Restore { vdf_ctx* c; int a; ~Restore() { vdf_ctx_sync(c); vdf_ctx_set_async(c, a); } } restore{ctx, was_async};
    // lockstep width: at most COMPRESS_LOCKSTEP proofs, fewer when the free HBM (less a reserve) does not hold their scratch
    const size_t per_proof = 32 * (spartan_scratch_elems(S1) + spartan_scratch_elems(S2) + S2.ncols + S2.num_cons);
    size_t width = COMPRESS_LOCKSTEP;
    {
      size_t free_b = 0, total_b = 0;
      HIPCALL(ctx, vdf_dev_mem_info(ctx, &free_b, &total_b));
      const size_t avail = free_b > COMPRESS_HBM_RESERVE ? free_b - COMPRESS_HBM_RESERVE : 0;
      width = std::max<size_t>(1, std::min(width, avail / per_proof));
    }
    std::vector<std::unique_ptr<vdf_snark>> snarks(uniq.size());
    std::lock_guard<std::mutex> aux_lock(pp->aux_mu);
    for (size_t g0 = 0; g0 < uniq.size(); g0 += width) {
      const size_t K = std::min(width, uniq.size() - g0);
      DevBufs bufs(ctx);
      std::vector<void*> d_fz(K), d_fE(K);
      std::vector<Inst> f2(K);
      std::vector<ProveIn> in1(K), in2(K);
      for (size_t q = 0; q < K; ++q) {
        const vdf_proof* p = uniq[g0 + q];
        snarks[g0 + q].reset(new vdf_snark());
        vdf_snark* s = snarks[g0 + q].get();
        { int rc = bufs.zeros(S2.ncols, &d_fz[q]); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
        { int rc = bufs.zeros(S2.num_cons, &d_fE[q]); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
        { int rc = compress_prelude(p, pp, s, d_fz[q], d_fE[q], &f2[q]); if (rc != VDF_OK) return rc; }
        in1[q] = {s->r_U1.comm_W, s->r_U1.comm_E, s->r_U1.u, s->r_U1.X, p->r[PRIMARY].d_z, p->r[PRIMARY].d_E, &s->sp[0]};
        in2[q] = {f2[q].comm_W, f2[q].comm_E, f2[q].u, f2[q].X, d_fz[q], d_fE[q], &s->sp[1]};
      }
      OwnedArena a1(ctx), a2(pp->aux_ctx ? pp->aux_ctx : ctx);
      if (K == 1) {                                                    // a group of one is the single prover's call
        int rc = prove_both_sides(pp, 1, in1.data(), in2.data(), &pp->arena[PRIMARY], &pp->arena[SECONDARY]);
        if (rc != VDF_OK) return rc;
      } else {
        { int rc = compress_queues(pp); if (rc != VDF_OK) return rc; }
        a2.ctx = pp->aux_ctx;
        int rc = prove_both_sides(pp, K, in1.data(), in2.data(), &a1, &a2);
        if (rc != VDF_OK) return rc;
      }
    }
    for (size_t q = 0; q < count; ++q) {
      const vdf_snark& s = *snarks[which[q]];
      out[q] = new vdf_snark(s);
    }
    return VDF_OK;
  });
}

void vdf_nova_snark_free(vdf_snark* s) { delete s; }

}  // extern "C"

namespace {

// The exact checks of one compressed proof (src/nova/proof.rs:383): the two output hashes, the carried z_i, the last fold of
// the instances, then each side's transcript replay; its four openings' group checks are left in d[side][W / E].  *ok =
// false when an exact check fails.  The caller has checked the parameters and made the context asynchronous.
int verify_replay(const vdf_snark* s, vdf_pp* pp, size_t num_steps, const vdf_fe* z0, const vdf_fe* zi, IpaDeferred d[2][2], bool* ok,
                  MDeferred* md = nullptr) {
  *ok = false;
  if (num_steps == 0) return VDF_OK;
  const Side& S1 = pp->s[PRIMARY];
  const Side& S2 = pp->s[SECONDARY];
  const Field& F1 = *S1.F;
  const Field& F2 = *S2.F;
  if (s->zi1.size() != pp->arity) return VDF_OK;
  const std::vector<Fe> z0p((const Fe*)z0, (const Fe*)z0 + pp->arity), z0s(1, zero()), zi1 = s->zi1, zi2(s->zi2, s->zi2 + 1);
  uint64_t hv[4];
  hash_state(S1.field, pp->params[PRIMARY], from_u64(num_steps, F1), z0p, zi1, to_relaxed(s->r_U2, F2), hv, pp->ro);
  if (int_to_fe(hv, F2) != s->l_u2.X[0]) return VDF_OK;
  hash_state(S2.field, pp->params[SECONDARY], from_u64(num_steps, F2), z0s, zi2, to_relaxed(s->r_U1, F1), hv, pp->ro);
  if (int_to_fe(hv, F2) != s->l_u2.X[1]) return VDF_OK;
  if (memcmp(s->zi1.data(), zi, 32 * pp->arity) != 0 || !s->zi2[0].is_zero()) return VDF_OK;       // src/nova/proof.rs:386
  uint64_t r[4];
  fold_challenge(pp, s->r_U2, s->l_u2, s->T2, r);
  const Inst f2 = fold_instance(S2, s->r_U2, s->l_u2, s->T2, r);
  bool good = false;
  // md (two entries, one per side): the replays stay on the host and leave their comparison with M(r_x, r_y) there
  int rc = md ? spartan_replay_host(S1, s->r_U1.comm_W, s->r_U1.comm_E, s->r_U1.u, s->r_U1.X, s->sp[0], d[0], &md[0], &good)
              : spartan_replay(S1, s->r_U1.comm_W, s->r_U1.comm_E, s->r_U1.u, s->r_U1.X, s->sp[0], d[0], &good);
  if (rc != VDF_OK || !good) return rc;
  rc = md ? spartan_replay_host(S2, f2.comm_W, f2.comm_E, f2.u, f2.X, s->sp[1], d[1], &md[1], &good)
          : spartan_replay(S2, f2.comm_W, f2.comm_E, f2.u, f2.X, s->sp[1], d[1], &good);
  if (rc != VDF_OK || !good) return rc;
  *ok = true;
  return VDF_OK;
}

// one compressed proof, every check at once (the single verifier)
int verify_one(const vdf_snark* s, vdf_pp* pp, size_t num_steps, const vdf_fe* z0, const vdf_fe* zi, bool* ok) {
  *ok = false;
  IpaDeferred d[2][2];
  bool good = false;
  { int rc = verify_replay(s, pp, num_steps, z0, zi, d, &good); if (rc != VDF_OK || !good) return rc; }
  for (int side = 0; side < 2; ++side) {
    const Side& sd = pp->s[side];
    DevBufs bufs(sd.ctx, sd.arena);
    const size_t n = std::max(d[side][0].n, d[side][1].n);
    void* d_s;
    { int rc = bufs.reserve(n); if (rc != VDF_OK) return fail(rc, vdf_last_error(sd.ctx)); }
    { int rc = bufs.zeros(n, &d_s); if (rc != VDF_OK) return fail(rc, vdf_last_error(sd.ctx)); }
    for (int q = 0; q < 2; ++q) {
      int rc = ipa_check_one(sd, d[side][q], d_s, &good);
      if (rc != VDF_OK || !good) return rc;
    }
  }
  *ok = true;
  return VDF_OK;
}

// The deferred checks of many openings of one side as one equation: with independent weights w_o,
//   MSM(G, sum_o w_o coefficients_o) == sum_o w_o (P_o + sum_j x_j^2 L_j + x_j^-2 R_j) + (sum_o w_o c_o (v_o - ab_o)) gen_u
// -- one coefficient launch and one MSM over the generators, one MSM over the uploaded small points (gen_u once).
int check_combined(const Side& sd, const std::vector<const IpaDeferred*>& ds, const std::vector<Fe>& w, bool* ok) {
  vdf_ctx* ctx = sd.ctx;
  const Field& F = *sd.F;
  const Field& Fb = *sd.Fb;
  *ok = false;
  const size_t cnt = ds.size();
  size_t n = 0, npts = 1;
  for (const IpaDeferred* d : ds) { n = std::max(n, d->n); npts += 1 + d->lr_pts.size(); }
  std::vector<vdf_ipa_opening> ops(cnt);
  std::vector<Aff> pts;
  std::vector<Fe> sc;
  pts.reserve(npts); sc.reserve(npts);
  Fe u_sc = zero();
  for (size_t o = 0; o < cnt; ++o) {
    const IpaDeferred& d = *ds[o];
    vdf_ipa_opening& op = ops[o];
    memcpy(&op.weight, &w[o], 32);
    op.k = d.k; op.log_m = d.log_m;
    op.lo = (const vdf_fe*)d.xis.data(); op.hi = (const vdf_fe*)d.xs.data(); op.pattern = (const vdf_fe*)d.a.data();
    pts.push_back(d.P); sc.push_back(w[o]);
    for (size_t j = 0; j < d.lr_pts.size(); ++j) { pts.push_back(d.lr_pts[j]); sc.push_back(mul(w[o], d.lr_sc[j], F)); }
    u_sc = add(u_sc, mul(w[o], mul(int_to_fe(d.q_raw, F), sub(d.v, d.ab, F), F), F), F);
  }
  pts.push_back(sd.gen_u); sc.push_back(u_sc);
  DevBufs bufs(ctx, sd.arena);
  void* d_c;
  { int rc = bufs.reserve(n); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
  { int rc = bufs.zeros(n, &d_c); if (rc != VDF_OK) return fail(rc, vdf_last_error(ctx)); }
  HIPCALL(ctx, vdf_ipa_coefficients(ctx, sd.field, ops.data(), (int)cnt, n, (vdf_fe*)d_c));
  vdf_jac jg, jp;
  HIPCALL(ctx, vdf_msm(ctx, sd.gens, 0, (const vdf_fe*)d_c, n, 1, &jg));
  { int rc = msm_points(sd, pts, sc, &jp); if (rc != VDF_OK) return rc; }
  HIPCALL(ctx, vdf_ctx_sync(ctx));
  const Aff a1 = jac_to_aff(jg, Fb), a2 = jac_to_aff(jp, Fb);
  *ok = memcmp(&a1, &a2, sizeof(Aff)) == 0;
  return VDF_OK;
}

}  // namespace

namespace vdfnova {

// sum_j sc[j] pts[j] over a few host points (Montgomery scalars) on the side's context: one upload, one MSM.  *out (host) is
// ready after vdf_ctx_sync.
int msm_points(const Side& sd, const std::vector<Aff>& pts, const std::vector<Fe>& sc, vdf_jac* out) {
  vdf_ctx* ctx = sd.ctx;
  vdf_bases* pb = nullptr;
  HIPCALL(ctx, vdf_bases_upload(ctx, sd.curve, (const vdf_affine*)pts.data(), pts.size(), &pb));
  const int rc = vdf_msm(ctx, pb, 0, (const vdf_fe*)sc.data(), pts.size(), 1, out);
  const std::string err = rc == VDF_OK ? "" : vdf_last_error(ctx);
  vdf_bases_free(pb);
  if (rc != VDF_OK) return fail(rc, "vdf_msm (small points): " + err);
  return VDF_OK;
}

// Points per pass of the batch verifier's M(r_x, r_y) for a new parameter set.  Shipped: 16 -- at t = 2^16 its slowest batch of 16
// was faster than the per-proof sequence's fastest, and a batch of one no slower (profiles/r21_verify_multi.txt;
// tools/gpu_verify_multi_time.py states the rule).
int verify_multi_default() {
  static const int v = [] {
    if (const char* e = env_override("VDF_NOVA_VERIFY_MULTI")) {
      char* end = nullptr;
      const long n = strtol(e, &end, 10);
      if (end != e && *end == 0 && n >= 0 && n <= VDF_SPARSE_EVAL_MAX) return (int)n;
    }
    return 16;
  }();
  return v;
}

}  // namespace vdfnova

namespace {
// ---- "VDFSNK03" read back: the one walk over the layout (include/vdf_nova.h) ----------------------------------------------------
// What stands in front of the elements: length, magic, t, digest.  The codes are vdf_nova_snark_deserialize's.  *L: both layouts.
int snark_wire_header(const vdf_pp* pp, const uint8_t* in, size_t len, Layout L[2]) {
  if (len < 48 + statement_wire(pp->arity)) return fail(VDF_ERR_BAD_LENGTH, "encoding is shorter than its header");
  if (memcmp(in, WIRE_MAGIC_SNARK, 8) != 0) return fail(VDF_ERR_BAD_ARG, "not this kind of encoding (magic)");
  uint64_t t;
  memcpy(&t, in + 8, 8);
  if (t != pp->t || memcmp(in + 16, pp->digest, 32) != 0) return fail(VDF_ERR_BAD_ARG, "encoding was made under other public parameters");
  L[0] = layout_of(pp->s[0]); L[1] = layout_of(pp->s[1]);
  if (len != 48 + statement_wire(pp->arity) + spartan_wire_size(L[0]) + spartan_wire_size(L[1]))
    return fail(VDF_ERR_BAD_LENGTH, "encoding has the wrong length for this shape");
  return VDF_OK;
}
// Every element behind a header that passed: field elements are range-checked and converted here (*canonical), every point's 32
// bytes go to point(enc, side, dst) with the place in the object they decode to -- the single call decodes them on the host as it
// walks, the batch call notes them and decodes all entries' points on the device.  The object's vectors are sized before any
// point is handed out and not again: dst stays valid for as long as the object does.
template <class PointFn>
std::unique_ptr<vdf_snark> snark_wire_walk(const vdf_pp* pp, const Layout L[2], const uint8_t* in, bool* canonical, PointFn&& point) {
  std::unique_ptr<vdf_snark> s(new vdf_snark());
  memcpy(&s->t, in + 8, 8);
  s->field = pp->field;
  memcpy(s->digest, pp->digest, 32);
  const uint8_t* i = in + 48;
  i = get_inst_points(i, &s->r_U1, pp->s[0], true, canonical, point);
  i = get_inst_points(i, &s->r_U2, pp->s[1], true, canonical, point);
  i = get_inst_points(i, &s->l_u2, pp->s[1], false, canonical, point);
  point(i, pp->s[1], &s->T2); i += 32;
  s->zi1.resize(pp->arity);
  for (size_t k = 0; k < pp->arity; ++k, i += 32) *canonical &= wire_get_fe(i, *pp->s[0].F, &s->zi1[k]);
  *canonical &= wire_get_fe(i, *pp->s[1].F, &s->zi2[0]); i += 32;
  for (int side = 0; side < 2; ++side) {
    const Field& F = *pp->s[side].F;
    Spartan& p = s->sp[side];
    spartan_resize(p, L[side]);
    auto get = [&](Fe& v) { *canonical &= wire_get_fe(i, F, &v); i += 32; };
    for (auto& ev : p.outer) for (Fe& v : ev) get(v);
    for (Fe& v : p.claims) get(v);
    for (auto& ev : p.inner) for (Fe& v : ev) get(v);
    get(p.w_eval);
    for (Ipa* ip : {&p.ipaW, &p.ipaE}) {
      for (size_t j = 0; j < ip->L.size(); ++j) {
        point(i, pp->s[side], &ip->L[j]);
        point(i + 32, pp->s[side], &ip->R[j]);
        i += 64;
      }
      for (Fe& v : ip->a) get(v);
    }
  }
  return s;
}
}  // namespace

extern "C" {

// verification of the compressed proof (src/nova/proof.rs:383): the two output hashes, the last fold of the instances,
// then one argument per side
int vdf_nova_verify_compressed(const vdf_snark* s, vdf_pp* pp, size_t num_steps, const vdf_fe z0[3], const vdf_fe zi[3], int* ok) {
  return nova_guard([&]() -> int {
    if (!s || !pp || !z0 || !zi || !ok) return fail(VDF_ERR_BAD_ARG, "null argument");
    *ok = 0;
    if (s->t != pp->t || memcmp(s->digest, pp->digest, 32) != 0) return fail(VDF_ERR_BAD_ARG, "proof was made under other public parameters");
    if (num_steps == 0) return VDF_OK;
    vdf_ctx* ctx = pp->ctx;
    int was_async = 0;
    HIPCALL(ctx, vdf_ctx_get_async(ctx, &was_async));
    HIPCALL(ctx, vdf_ctx_sync(ctx));
    HIPCALL(ctx, vdf_ctx_set_async(ctx, 1));
    struct Restore { vdf_ctx* c; int a; ~Restore() { vdf_ctx_sync(c); vdf_ctx_set_async(c, a); } } restore{ctx, was_async};
    bool good = false;
    int rc = verify_one(s, pp, num_steps, z0, zi, &good);
    if (rc != VDF_OK) return rc;
    *ok = good ? 1 : 0;
    return VDF_OK;
  });
}

// Many compressed proofs under one parameter set: every proof's exact checks and transcript replay, then its openings' group
// checks combined per side with 128-bit weights drawn from a transcript of the whole batch -- the weights depend on every
// proof, statement and step count, so errors in two proofs cannot be made to cancel.  When a combined check fails, the
// single verifier decides each remaining entry.
int vdf_nova_verify_compressed_batch(vdf_pp* pp, size_t count, const vdf_snark* const snarks[], const size_t num_steps[],
                                     const vdf_fe* z0, const vdf_fe* zi, int ok[], int* all_ok) {
  return nova_guard([&]() -> int {
    if (!pp || !all_ok) return fail(VDF_ERR_BAD_ARG, "null argument");
    *all_ok = 0;
    if (count == 0) { *all_ok = 1; return VDF_OK; }
    if (!snarks || !num_steps || !z0 || !zi || !ok) return fail(VDF_ERR_BAD_ARG, "null argument");
    for (size_t q = 0; q < count; ++q) ok[q] = 0;
    for (size_t q = 0; q < count; ++q) {
      const vdf_snark* s = snarks[q];
      if (!s) return fail(VDF_ERR_BAD_ARG, "entry " + std::to_string(q) + ": null proof");
      if (s->t != pp->t || memcmp(s->digest, pp->digest, 32) != 0)
        return fail(VDF_ERR_BAD_ARG, "entry " + std::to_string(q) + ": proof was made under other public parameters");
    }
    const size_t ar = pp->arity;
    // the weights' transcript: the parameters, then every entry in full
    Transcript tw("verify-batch");
    tw.absorb("pp", pp->digest, 32);
    { const uint64_t c = count; tw.absorb("count", &c, 8); }
    std::vector<uint8_t> buf;
    for (size_t q = 0; q < count; ++q) {
      buf.resize(vdf_nova_snark_serialized_size(snarks[q]));
      { int rc = vdf_nova_snark_serialize(snarks[q], buf.data(), buf.size()); if (rc != VDF_OK) return rc; }
      tw.absorb("proof", buf.data(), buf.size());
      const uint64_t st = num_steps[q];
      tw.absorb("steps", &st, 8);
      tw.absorb("z0", z0 + q * ar, 32 * ar);
      tw.absorb("zi", zi + q * ar, 32 * ar);
    }
    vdf_ctx* ctx = pp->ctx;
    int was_async = 0;
    HIPCALL(ctx, vdf_ctx_get_async(ctx, &was_async));
    HIPCALL(ctx, vdf_ctx_sync(ctx));
    HIPCALL(ctx, vdf_ctx_set_async(ctx, 1));
    struct Restore { vdf_ctx* c; int a; ~Restore() { vdf_ctx_sync(c); vdf_ctx_set_async(c, a); } } restore{ctx, was_async};
    // exact checks and replays; an entry that fails one leaves the batch
    // verify_multi = n > 0: the replays run on the host alone, and every live entry's M(r_x, r_y) is evaluated afterwards, at
    // most n points per pass over a side's shape (spartan_m_check); 0: each replay evaluates its own, as the single verifier does
    const size_t multi = (size_t)pp->verify_multi.load();
    std::vector<std::array<std::array<IpaDeferred, 2>, 2>> d(count);
    std::vector<std::array<MDeferred, 2>> md(multi ? count : 0);
    std::vector<size_t> live;
    for (size_t q = 0; q < count; ++q) {
      IpaDeferred dq[2][2];
      bool good = false;
      int rc = verify_replay(snarks[q], pp, num_steps[q], z0 + q * ar, zi + q * ar, dq, &good, multi ? md[q].data() : nullptr);
      if (rc != VDF_OK) return rc;
      if (!good) continue;
      for (int side = 0; side < 2; ++side)
        for (int o = 0; o < 2; ++o) d[q][side][o] = std::move(dq[side][o]);
      live.push_back(q);
    }
    for (int side = 0; multi && side < 2 && !live.empty(); ++side) {
      std::vector<const MDeferred*> items;
      for (size_t q : live) items.push_back(&md[q][side]);
      std::unique_ptr<bool[]> good(new bool[items.size()]);
      uint64_t st[3] = {0, 0, 0};
      int rc = spartan_m_check(pp->s[side], items.data(), items.size(), multi, good.get(), st);
      for (int k = 0; k < 3; ++k) pp->verify_multi_stats[k] += st[k];
      if (rc != VDF_OK) return rc;
      std::vector<size_t> still;
      for (size_t k = 0; k < live.size(); ++k) if (good[k]) still.push_back(live[k]);
      live.swap(still);
    }
    // one weight per opening: entry by entry, side by side, W then E (drawn for every entry, so that the weights of an
    // entry do not depend on which others failed)
    std::vector<std::array<std::array<Fe, 2>, 2>> w(count);
    uint64_t raw[4];
    for (size_t q = 0; q < count; ++q)
      for (int side = 0; side < 2; ++side)
        for (int o = 0; o < 2; ++o) w[q][side][o] = tw.challenge("weight", *pp->s[side].F, raw);
    bool combined = true;
    if (!live.empty())
      for (int side = 0; side < 2 && combined; ++side) {
        std::vector<const IpaDeferred*> ds;
        std::vector<Fe> ws;
        for (size_t q : live)
          for (int o = 0; o < 2; ++o) { ds.push_back(&d[q][side][o]); ws.push_back(w[q][side][o]); }
        int rc = check_combined(pp->s[side], ds, ws, &combined);
        if (rc != VDF_OK) return rc;
      }
    if (combined) {
      for (size_t q : live) ok[q] = 1;
    } else {
      for (size_t q : live) {                                         // attribution: each remaining entry on its own
        bool good = false;
        int rc = verify_one(snarks[q], pp, num_steps[q], z0 + q * ar, zi + q * ar, &good);
        if (rc != VDF_OK) return rc;
        ok[q] = good ? 1 : 0;
      }
    }
    int all = 1;
    for (size_t q = 0; q < count; ++q) all &= ok[q];
    *all_ok = all;
    return VDF_OK;
  });
}

// flat canonical encoding of the two arguments (little-endian, non-Montgomery), primary then secondary; per argument:
// outer rounds (3 each), 4 claims, inner rounds (2 each), w, then per opening (L, R) per round as affine (x, y) and the
// final vector (at most 16 elements)
size_t vdf_nova_snark_size(const vdf_snark* s) { return s ? spartan_flat_size(s->sp[0]) + spartan_flat_size(s->sp[1]) : 0; }

int vdf_nova_snark_bytes(const vdf_snark* s, uint8_t* out, size_t cap) {
  return nova_guard([&]() -> int {
    if (!s || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (cap < vdf_nova_snark_size(s)) return fail(VDF_ERR_BAD_LENGTH, "buffer too small");
    uint8_t* o = out;
    for (int side = 0; side < 2; ++side) {
      const Field& F = field(cycle_field(s->field, side));
      const Field& Fb = field(cycle_field(s->field, 1 - side));
      const Spartan& sp = s->sp[side];
      auto put = [&](const Fe& v, const Field& f) { const Fe c = from_mont(v, f); memcpy(o, c.l, 32); o += 32; };
      auto put_pt = [&](const Aff& a) { if (a.is_id()) { memset(o, 0, 64); o += 64; } else { put(a.x, Fb); put(a.y, Fb); } };
      for (const auto& ev : sp.outer) for (const Fe& v : ev) put(v, F);
      for (const Fe& v : sp.claims) put(v, F);
      for (const auto& ev : sp.inner) for (const Fe& v : ev) put(v, F);
      put(sp.w_eval, F);
      for (const Ipa* ip : {&sp.ipaW, &sp.ipaE}) {
        for (size_t j = 0; j < ip->L.size(); ++j) { put_pt(ip->L[j]); put_pt(ip->R[j]); }
        for (const Fe& v : ip->a) put(v, F);
      }
    }
    return VDF_OK;
  });
}

// replaces both arguments by the given encoding (the tests use it to tamper): field elements must be canonical and
// every point the identity or on its curve
int vdf_nova_snark_set_bytes(vdf_snark* s, const uint8_t* in, size_t len) {
  return nova_guard([&]() -> int {
    if (!s || !in) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (len != vdf_nova_snark_size(s)) return fail(VDF_ERR_BAD_LENGTH, "encoding has the wrong length for this shape");
    const uint8_t* i = in;
    bool canonical = true, on_curve = true;
    Spartan tmp[2] = {s->sp[0], s->sp[1]};
    for (int side = 0; side < 2; ++side) {
      const Field& F = field(cycle_field(s->field, side));
      const Field& Fb = field(cycle_field(s->field, 1 - side));
      Spartan& sp = tmp[side];
      auto get = [&](Fe& v, const Field& f) { Fe c; memcpy(c.l, i, 32); i += 32; if (geq(c.l, f.m)) canonical = false; v = to_mont(c, f); };
      auto get_pt = [&](Aff& a) {
        get(a.x, Fb); get(a.y, Fb);
        if (!a.is_id() && sqr(a.y, Fb) != add(mul(sqr(a.x, Fb), a.x, Fb), from_u64(5, Fb), Fb)) on_curve = false;
      };
      for (auto& ev : sp.outer) for (Fe& v : ev) get(v, F);
      for (Fe& v : sp.claims) get(v, F);
      for (auto& ev : sp.inner) for (Fe& v : ev) get(v, F);
      get(sp.w_eval, F);
      for (Ipa* ip : {&sp.ipaW, &sp.ipaE}) {
        for (size_t j = 0; j < ip->L.size(); ++j) { get_pt(ip->L[j]); get_pt(ip->R[j]); }
        for (Fe& v : ip->a) get(v, F);
      }
    }
    if (!canonical) return fail(VDF_ERR_NONCANONICAL, "a field element of the encoding is not canonical");
    if (!on_curve) return fail(VDF_ERR_NONCANONICAL, "a point of the encoding is not on its curve");
    s->sp[0] = tmp[0]; s->sp[1] = tmp[1];
    return VDF_OK;
  });
}

// ---- the whole compressed proof as one byte string ("VDFSNK03", layout in include/vdf_nova.h) -----------------------
size_t vdf_nova_snark_serialized_size(const vdf_snark* s) {
  if (!s) return 0;
  size_t n = 8 + 8 + 32 + statement_wire(s->zi1.size());
  for (const Spartan& p : s->sp)
    n += 32 * (3 * p.outer.size() + 4 + 2 * p.inner.size() + 1 + p.ipaW.a.size() + p.ipaE.a.size()) + 64 * (p.ipaW.L.size() + p.ipaE.L.size());
  return n;
}

int vdf_nova_snark_serialize(const vdf_snark* s, uint8_t* out, size_t cap) {
  return nova_guard([&]() -> int {
    if (!s || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (cap < vdf_nova_snark_serialized_size(s)) return fail(VDF_ERR_BAD_LENGTH, "buffer too small");
    Side sd[2];
    for (int k = 0; k < 2; ++k) { sd[k].F = &field(cycle_field(s->field, k)); sd[k].Fb = &field(cycle_field(s->field, 1 - k)); }
    uint8_t* o = out;
    memcpy(o, WIRE_MAGIC_SNARK, 8); o += 8;
    memcpy(o, &s->t, 8); o += 8;
    memcpy(o, s->digest, 32); o += 32;
    o = put_inst(o, s->r_U1, sd[0], true);
    o = put_inst(o, s->r_U2, sd[1], true);
    o = put_inst(o, s->l_u2, sd[1], false);
    pt_compress(s->T2, *sd[1].Fb, o); o += 32;
    for (const Fe& v : s->zi1) o = wire_put_fe(o, v, *sd[0].F);
    o = wire_put_fe(o, s->zi2[0], *sd[1].F);
    for (int side = 0; side < 2; ++side) {
      const Field& F = *sd[side].F;
      const Field& Fb = *sd[side].Fb;
      const Spartan& sp = s->sp[side];
      for (const auto& ev : sp.outer) for (const Fe& v : ev) o = wire_put_fe(o, v, F);
      for (const Fe& v : sp.claims) o = wire_put_fe(o, v, F);
      for (const auto& ev : sp.inner) for (const Fe& v : ev) o = wire_put_fe(o, v, F);
      o = wire_put_fe(o, sp.w_eval, F);
      for (const Ipa* ip : {&sp.ipaW, &sp.ipaE}) {
        for (size_t j = 0; j < ip->L.size(); ++j) { pt_compress(ip->L[j], Fb, o); pt_compress(ip->R[j], Fb, o + 32); o += 64; }
        for (const Fe& v : ip->a) o = wire_put_fe(o, v, F);
      }
    }
    return VDF_OK;
  });
}

// A verifier that never saw the prover's objects: bytes -> vdf_snark
int vdf_nova_snark_deserialize(vdf_pp* pp, const uint8_t* in, size_t len, vdf_snark** out) {
  return nova_guard([&]() -> int {
    if (!pp || !in || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    Layout L[2];
    { int rc = snark_wire_header(pp, in, len, L); if (rc != VDF_OK) return rc; }
    bool canonical = true, on_curve = true;
    std::unique_ptr<vdf_snark> s = snark_wire_walk(pp, L, in, &canonical, [&](const uint8_t* enc, const Side& sd, Aff* dst) {
      on_curve &= pt_decompress(enc, *sd.Fb, dst);
    });
    if (!canonical) return fail(VDF_ERR_NONCANONICAL, "a field element of the encoding is not canonical");
    if (!on_curve) return fail(VDF_ERR_NONCANONICAL, "a point of the encoding does not decode to a curve point");
    *out = s.release();
    return VDF_OK;
  });
}

// Many encodings under one parameter set: the same header checks and the same walk per entry, the points of every entry that
// passed them decoded by one vdf_points_decompress per curve (side 0's commitments lie on pp->s[0].curve, side 1's on the other)
// on a pinned block the kernels read and write in place, one wait, and the points scattered to where the walk said they go.
int vdf_nova_snark_deserialize_batch(vdf_pp* pp, size_t count, const uint8_t* const in[], const size_t len[], vdf_snark* out[],
                                     int status[]) {
  return nova_guard([&]() -> int {
    if (!pp || (count && (!in || !len || !out || !status))) return fail(VDF_ERR_BAD_ARG, "null argument");
    for (size_t q = 0; q < count; ++q) out[q] = nullptr;
    struct WirePoint { const uint8_t* enc; Aff* dst; size_t entry; };
    std::vector<WirePoint> pts[2];
    std::vector<std::unique_ptr<vdf_snark>> made(count);
    for (size_t q = 0; q < count; ++q) {
      if (!in[q]) { status[q] = fail(VDF_ERR_BAD_ARG, "null argument"); continue; }
      Layout L[2];
      status[q] = snark_wire_header(pp, in[q], len[q], L);
      if (status[q] != VDF_OK) continue;
      const size_t mark[2] = {pts[0].size(), pts[1].size()};
      bool canonical = true;
      made[q] = snark_wire_walk(pp, L, in[q], &canonical, [&](const uint8_t* enc, const Side& sd, Aff* dst) {
        pts[&sd - pp->s].push_back({enc, dst, q});
      });
      if (!canonical) {                                  // it leaves with its points: they are not decoded
        status[q] = fail(VDF_ERR_NONCANONICAL, "a field element of the encoding is not canonical");
        made[q].reset();
        pts[0].resize(mark[0]); pts[1].resize(mark[1]);
      }
    }
    const size_t n[2] = {pts[0].size(), pts[1].size()}, total = n[0] + n[1];
    if (total) {
      vdf_ctx* ctx = pp->ctx;
      // [enc: 32 total | points: 64 total | ok: total], side 0's share of each first
      void* blk = nullptr;
      HIPCALL(ctx, vdf_host_alloc(ctx, 97 * total, &blk));
      struct Free { vdf_ctx* c; void* p; ~Free() { vdf_host_free(c, p); } } free_blk{ctx, blk};
      uint8_t* enc = static_cast<uint8_t*>(blk);
      vdf_affine* dec = reinterpret_cast<vdf_affine*>(enc + 32 * total);
      uint8_t* good = enc + 96 * total;
      {
        uint8_t* e = enc;
        for (int side = 0; side < 2; ++side)
          for (const WirePoint& w : pts[side]) { memcpy(e, w.enc, 32); e += 32; }
      }
      {
        int was_async = 0;
        HIPCALL(ctx, vdf_ctx_get_async(ctx, &was_async));
        HIPCALL(ctx, vdf_ctx_set_async(ctx, 1));
        struct Restore { vdf_ctx* c; int a; ~Restore() { vdf_ctx_sync(c); vdf_ctx_set_async(c, a); } } restore{ctx, was_async};
        for (int side = 0; side < 2; ++side) {
          const size_t at = side ? n[0] : 0;
          HIPCALL(ctx, vdf_points_decompress(ctx, pp->s[side].curve, enc + 32 * at, n[side], dec + at, good + at));
        }
        HIPCALL(ctx, vdf_ctx_sync(ctx));
      }
      size_t k = 0;
      for (int side = 0; side < 2; ++side)
        for (const WirePoint& w : pts[side])
          if (!good[k++] && made[w.entry]) {
            status[w.entry] = fail(VDF_ERR_NONCANONICAL, "a point of the encoding does not decode to a curve point");
            made[w.entry].reset();
          }
      k = 0;
      for (int side = 0; side < 2; ++side)
        for (const WirePoint& w : pts[side]) {
          if (made[w.entry]) memcpy(w.dst, &dec[k], sizeof(Aff));
          ++k;
        }
    }
    for (size_t q = 0; q < count; ++q) out[q] = made[q].release();
    return VDF_OK;
  });
}

// Bytes in, verdicts out: vdf_nova_snark_deserialize_batch, then vdf_nova_verify_compressed_batch over the entries that decoded.
int vdf_nova_verify_wire_batch(vdf_pp* pp, size_t count, const uint8_t* const in[], const size_t len[], const size_t num_steps[],
                               const vdf_fe* z0, const vdf_fe* zi, int ok[], int status[], int* all_ok) {
  return nova_guard([&]() -> int {
    if (!pp || !all_ok) return fail(VDF_ERR_BAD_ARG, "null argument");
    *all_ok = 0;
    if (count == 0) { *all_ok = 1; return VDF_OK; }
    if (!in || !len || !num_steps || !z0 || !zi || !ok || !status) return fail(VDF_ERR_BAD_ARG, "null argument");
    for (size_t q = 0; q < count; ++q) ok[q] = 0;
    struct Handles {
      std::vector<vdf_snark*> v;
      ~Handles() { for (vdf_snark* s : v) delete s; }
    } hs{std::vector<vdf_snark*>(count, nullptr)};
    { int rc = vdf_nova_snark_deserialize_batch(pp, count, in, len, hs.v.data(), status); if (rc != VDF_OK) return rc; }
    const size_t ar = pp->arity;
    std::vector<size_t> live, steps;
    std::vector<const vdf_snark*> snarks;
    std::vector<vdf_fe> lz0, lzi;
    for (size_t q = 0; q < count; ++q) {
      if (!hs.v[q]) continue;
      live.push_back(q);
      snarks.push_back(hs.v[q]);
      steps.push_back(num_steps[q]);
      lz0.insert(lz0.end(), z0 + q * ar, z0 + (q + 1) * ar);
      lzi.insert(lzi.end(), zi + q * ar, zi + (q + 1) * ar);
    }
    std::vector<int> okl(live.size(), 0);
    int all = 1;
    if (!live.empty()) {
      int rc = vdf_nova_verify_compressed_batch(pp, live.size(), snarks.data(), steps.data(), lz0.data(), lzi.data(), okl.data(), &all);
      if (rc != VDF_OK) return rc;
    }
    for (size_t k = 0; k < live.size(); ++k) ok[live[k]] = okl[k];
    *all_ok = (all && live.size() == count) ? 1 : 0;
    return VDF_OK;
  });
}

// ---- how many points of a shape one pass of the batch verifier evaluates (include/vdf_nova.h) ------------------------
int vdf_nova_pp_set_verify_multi(vdf_pp* pp, int n) {
  if (!pp) return fail(VDF_ERR_BAD_ARG, "null argument");
  if (n < 0 || n > VDF_SPARSE_EVAL_MAX) return fail(VDF_ERR_BAD_ARG, "verify_multi must be 0..64");
  pp->verify_multi.store(n);
  return VDF_OK;
}
int vdf_nova_pp_verify_multi(const vdf_pp* pp) { return pp ? pp->verify_multi.load() : 0; }
int vdf_nova_pp_verify_multi_stats(const vdf_pp* pp, uint64_t out[3]) {
  if (!pp || !out) return fail(VDF_ERR_BAD_ARG, "null argument");
  for (int k = 0; k < 3; ++k) out[k] = pp->verify_multi_stats[k].load();
  return VDF_OK;
}

}  // extern "C"
