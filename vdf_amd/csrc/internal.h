// Internal declarations shared by the translation units of libvdf_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/vdf_hip.h"
#include "pasta_constants.h"

namespace vdf {
// Per-launch timing for the roofline report (vdf_ctx_set_kernel_timing): a launch site constructs a KTimer around its
// launch; when the calling thread has a sink (set by the ABI's guard while the context's kernel timing is on) two HIP
// events bracket the launch on its stream.  Off by default: no events, no cost.
struct KRecord { const char* name; double bytes; hipEvent_t e0, e1; };
struct KSink {
  std::vector<KRecord> rec;
  std::vector<hipEvent_t> pool;
};
extern thread_local KSink* tl_ksink;
struct KTimer {
  hipStream_t s; KSink* k; KRecord r;
  KTimer(hipStream_t st, const char* name, double bytes) : s(st), k(tl_ksink) {
    if (!k) return;
    r.name = name; r.bytes = bytes; r.e0 = r.e1 = nullptr;
    for (hipEvent_t* e : {&r.e0, &r.e1}) {
      if (!k->pool.empty()) { *e = k->pool.back(); k->pool.pop_back(); }
      else if (hipEventCreate(e) != hipSuccess) { (void)hipGetLastError(); *e = nullptr; }
    }
    if (r.e0 && r.e1) (void)hipEventRecord(r.e0, s); else k = nullptr;
  }
  ~KTimer() {
    if (!k) return;
    (void)hipEventRecord(r.e1, s);
    k->rec.push_back(r);
  }
  KTimer(const KTimer&) = delete;
  KTimer& operator=(const KTimer&) = delete;
};
}  // namespace vdf

namespace vdf { const vdf_hip_tuning& tuning(); }     // process-wide tuning (abi.hip), environment overrides applied once

// A caller context's stream and the two streams opened right behind it (abi.hip: the hardware maps queues to its pipes in the
// order they were created, and a prover whose three queues are neighbours runs 10-14 % faster than one whose queues are not)
struct vdf_queue_family {
  int device = 0;
  static constexpr int N = 3;
  hipStream_t s[N] = {};
  bool used[N] = {};
  ~vdf_queue_family();
};

struct vdf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int pool_slot = -1;                // >= 0: the stream belongs to the device's pool of hardware queues (vdf_ctx_create_pooled)
  std::shared_ptr<vdf_queue_family> family;   // the stream is family->s[family_idx] (vdf_ctx_create: 0; vdf_ctx_create_pooled_near: 1, 2)
  int family_idx = -1;
  bool foreign_stream = false;       // vdf_ctx_set_stream put a caller's stream in place of the context's own
  bool async = false;
  int msm_window = 0;          // 0 = automatic
  std::mutex mu;
  std::string err;
  // MSM workspace (grown on demand, reused across calls)
  void* ws = nullptr;
  size_t ws_bytes = 0;
  void* d_out = nullptr;       // 128 B result slot
  static constexpr size_t SMALL_POOL_BYTES = 16 * 1024;
  void* small_pool = nullptr;  // staging for tiny host operands (challenge scalars, result points)
  static constexpr size_t PINNED_OUT_BYTES = 256;
  void* h_out = nullptr;       // pinned host memory mapped into the device: result slot kernels write directly
  void* h_out_dev = nullptr;   // its device-side address
  int num_cus = 256;
  // stage timing (bench.py roofline leg)
  bool timing = false;
  bool ktiming = false;              // per-launch events (vdf_ctx_set_kernel_timing)
  vdf::KSink ksink;
  struct TimedCall { hipEvent_t ev[4]; };
  std::vector<TimedCall> timed;      // events of calls not yet queried
  std::vector<hipEvent_t> ev_pool;   // recycled events
  hipEvent_t wait_ev = nullptr;      // vdf_ctx_wait
  hipEvent_t marks[VDF_MARK_SLOTS] = {};                          // vdf_ctx_mark (0..3 the caller's, 4..15 libvdf_nova.so's)
  // MSM jobs (vdf_msm_job_*): one side stream and two events per vector, created on first use
  hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t side_go[4] = {nullptr, nullptr, nullptr, nullptr}, side_done[4] = {nullptr, nullptr, nullptr, nullptr};
  bool job_open = false;
  void* reduce_scratch = nullptr;    // per-workgroup partial sums of vdf_reduce
  void* eval_scratch = nullptr;      // vdf_sparse_eval_multi: count results, then its per-workgroup partial sums (grown on demand)
  size_t eval_scratch_bytes = 0;
  void* ipa_host = nullptr;          // vdf_ipa_coefficients: the openings' factors packed in pinned memory ...
  void* ipa_dev = nullptr;           // ... and their device copy, ipa_cap bytes each (grown on demand)
  size_t ipa_cap = 0;
  hipEvent_t ipa_copied = nullptr;   // the last copy out of ipa_host has been made
  int acc_fill = 0;                  // accumulate workgroups per CU this context's MSMs fill (vdf_ctx_set_accumulate_fill; 0 = process-wide)
  int light_prio = 3;                // wave priority of this context's sort / bucket-reduction kernels (vdf_ctx_set_light_priority)
  hipEvent_t acc_gate = nullptr;     // one-shot: the next bucket-method MSM's accumulation waits for this event (vdf_ctx_gate_accumulate)
  void* glv_scalars = nullptr;       // 2n half-scalars of the endomorphism's split (table-less MSMs over a whole generator set)
  size_t glv_bytes = 0;
  void* glv_pts = nullptr;           // [P | phi(P)] of an EPHEMERAL generator set (the uncached shims): scratch, reused call after call
  size_t glv_pts_bytes = 0;
  uint32_t* direct_arrived = nullptr;  // MSM_MAX_GROUPS counters of the direct sum's last-arriver step (zero between calls)
};

struct vdf_bases {
  vdf_ctx* ctx = nullptr;
  int curve = 0;
  size_t n = 0;
  void* d_pts = nullptr;       // n affine points, 64 B each
  void* d_pts2 = nullptr;      // [P | phi(P)], 2n points: made by the first table-less MSM over the whole set (abi.hip msm_core)
  std::mutex glv_mu;
  bool ephemeral = false;      // made for one call (abi.hip shim): nothing derived from it is worth keeping
  // fixed-base table: tables x n affine points; table j holds 2^(c*sets*j) * P_i
  int tbl_c = 0, tbl_sets = 0, tbl_tables = 0;
  void* d_table = nullptr;
  // digit table (vdf_bases_precompute_digits, msm_direct.hip): every multiple d * 2^(c j) of the generators in up to 4
  // index ranges; range r holds slots [dg_slot0[r], dg_slot0[r] + dg_count[r])
  int dg_c = 0, dg_ranges = 0;
  size_t dg_begin[4] = {0, 0, 0, 0}, dg_count[4] = {0, 0, 0, 0}, dg_slot0[4] = {0, 0, 0, 0};
  void* d_digits = nullptr;
  size_t dg_bytes = 0;
};

struct vdf_shape {
  vdf_ctx* ctx = nullptr;
  int field = 0;
  size_t num_cons = 0, num_cols = 0;
  size_t nnz[3] = {0, 0, 0};
  uint32_t* d_rowptr[3] = {nullptr, nullptr, nullptr};   // num_cons + 1
  uint32_t* d_col[3] = {nullptr, nullptr, nullptr};      // nnz
  uint32_t* d_coef[3] = {nullptr, nullptr, nullptr};     // nnz, index into dictionary
  void* d_dict = nullptr;                                 // dictionary of field elements
  size_t dict_len = 0;
  // the three matrices merged in column-major order (vdf_spmv3_t): entry = (row, coefficient index | matrix << 30)
  uint32_t* d_t_colptr = nullptr;                         // num_cols + 1
  uint32_t* d_t_row = nullptr;                            // nnz[0] + nnz[1] + nnz[2]
  uint32_t* d_t_cm = nullptr;
  uint32_t* d_t_heavy = nullptr;                          // columns with more than 64 entries
  size_t t_nheavy = 0, t_nbig = 0;                        // ... sorted longest first; the first t_nbig have more than 4096
  // rows with more than VDF_LONG_ROW entries, as row | matrix << 30: one wavefront each (vec_spmv_long) instead of one lane
  uint32_t* d_long = nullptr;
  size_t n_long = 0;
  // the distinct rows among them, ascending: one wavefront each in the fused cross term (k_nifs_cross_f)
  uint32_t* d_long_rowlist = nullptr;
  size_t n_long_rowlist = 0;
  std::vector<uint64_t> h_nnz_prefix;                     // entries of A + B + C in the rows above r (pricing of a row range)
  std::vector<uint32_t> h_long_rows;                      // ... their row numbers, ascending (vdf_nifs_cross_term_rows)
};
// A row of more than this many entries is summed by a whole wavefront ahead of the lane-per-row kernels, which then
// only read the result: the rows of an augmented circuit that pack 255 bits or carry a Poseidon state of ~60 terms would
// otherwise serialise a launch behind one lane (1 ms instead of 20 us at t = 2^16).
#define VDF_LONG_ROW 8

namespace vdf {

struct Status {
  int code = VDF_OK;
  std::string msg;
  bool ok() const { return code == VDF_OK; }
};

inline Status hip_status(hipError_t e, const char* what) {
  Status s;
  if (e != hipSuccess) {
    s.code = (e == hipErrorOutOfMemory) ? VDF_ERR_OOM : VDF_ERR_DEVICE;
    s.msg = std::string(what) + ": " + hipGetErrorString(e);
  }
  return s;
}

#define VDF_TRY_HIP(expr)                                   \
  do {                                                      \
    hipError_t e__ = (expr);                                \
    if (e__ != hipSuccess) return ::vdf::hip_status(e__, #expr); \
  } while (0)
#define VDF_TRY(expr)                 \
  do {                                \
    ::vdf::Status s__ = (expr);       \
    if (!s__.ok()) return s__;        \
  } while (0)

// ---- run-time field / curve -> template argument -----------------------------------------
// Every kernel is a template over the field (FpParams / FqParams, pasta_constants.h); this is the one way a launcher gets
// from an `int field` or `int curve` to that argument.  The body is a generic lambda over tags:
//   return with_field(field, [&](auto f) { hipLaunchKernelGGL((k_axpy<tag_t<decltype(f)>>), ...); });
// A body that returns void is a plain launch and is followed by the hipGetLastError() check here; a body that returns a
// Status (a launcher that is itself a template, or one with several checked steps) has its Status passed on.
template <class P> struct FieldTag { using type = P; };
template <class Tag> using tag_t = typename Tag::type;
constexpr int field_id(FieldTag<FpParams>) { return VDF_FIELD_FP; }
constexpr int field_id(FieldTag<FqParams>) { return VDF_FIELD_FQ; }

template <class F, class... Tags> Status dispatch_body(F&& f, Tags... tags) {
  if constexpr (std::is_void<decltype(f(tags...))>::value) {
    f(tags...);
    VDF_TRY_HIP(hipGetLastError());
    return Status{};
  } else {
    return f(tags...);
  }
}

template <class F> Status with_field(int field, F&& f) {
  if (field == VDF_FIELD_FP) return dispatch_body(f, FieldTag<FpParams>{});
  if (field == VDF_FIELD_FQ) return dispatch_body(f, FieldTag<FqParams>{});
  return Status{VDF_ERR_BAD_ARG, "unknown field"};
}
// f(base, scalar): the field of a curve's coordinates and the field of its scalars.  THE table of the Pasta cycle, stated
// here and nowhere else: Pallas = (Fp coordinates, Fq scalars), Vesta = (Fq coordinates, Fp scalars).
template <class F> Status with_curve(int curve, F&& f) {
  if (curve == VDF_CURVE_PALLAS) return dispatch_body(f, FieldTag<FpParams>{}, FieldTag<FqParams>{});
  if (curve == VDF_CURVE_VESTA) return dispatch_body(f, FieldTag<FqParams>{}, FieldTag<FpParams>{});
  return Status{VDF_ERR_BAD_ARG, "unknown curve"};
}
// the checks alone, for an entry point that allocates, uploads or caches something before its first launch
inline Status check_field(int field) { return with_field(field, [](auto) { return Status{}; }); }
inline Status check_curve(int curve) { return with_curve(curve, [](auto, auto) { return Status{}; }); }
// VDF_FIELD_* of a curve's scalars (-1: unknown curve)
inline int field_of_curve_scalar(int curve) {
  int field = -1;
  (void)with_curve(curve, [&](auto, auto scalar) { field = field_id(scalar); return Status{}; });
  return field;
}
// A small compile-time integer (a reduction kind, variables per round, lanes per row, a batch width) from its run-time
// value: f(std::integral_constant<int, V>{}) for the V of the list that equals v, under the same void / Status rule; a value
// outside the list is VDF_ERR_BAD_ARG with the site's own message.  Only the listed values are instantiated, in the order of
// the list (the kernels of a code object lie in the order of their instantiation).
template <int... Vs, class F> Status with_int(int v, const char* otherwise, F&& f) {
  Status st{VDF_ERR_BAD_ARG, otherwise};
  (void)(... || (v == Vs && ((st = dispatch_body(f, std::integral_constant<int, Vs>{})), true)));
  return st;
}
template <class F> Status with_bool(bool v, F&& f) {
  return v ? dispatch_body(f, std::true_type{}) : dispatch_body(f, std::false_type{});
}

// device vectors travel through the ABI as void*; the kernels take bytes
inline const char* cbytes_of(const void* p) { return static_cast<const char*>(p); }
inline char* bytes_of(void* p) { return static_cast<char*>(p); }
inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }     // one lane per element, workgroups of 256

// ---- msm.hip --------------------------------------------------------------------------
constexpr int MSM_MAX_GROUPS = 4;
// A plan covers a BATCH of 1..4 independent MSMs ("groups") over the same generator table: each group has its
// own scalar vector, length and generator offset and yields its own point.  The groups share every launch
// (one sort, one accumulate grid balanced over all entries, one latency-bound tail); to everything after pass A
// a group is simply `sets` more bucket sets.
struct MsmPlan {
  int groups = 1;
  uint32_t gn[MSM_MAX_GROUPS] = {0, 0, 0, 0};       // points per group
  uint32_t goff[MSM_MAX_GROUPS] = {0, 0, 0, 0};     // generator offset per group (points)
  uint32_t gblk_end[MSM_MAX_GROUPS] = {0, 0, 0, 0}; // pass-A workgroups: group g owns [gblk_end[g-1], gblk_end[g])
  uint32_t n = 0;        // points, all groups
  int c = 0;             // window bits
  int windows = 0;       // ceil(256 / c)  (ceil(132 / c) for the endomorphism's half-scalars)
  bool signed_scalars = false;   // the scalars are sign-and-magnitude words (k_glv_split)
  int sets = 0;          // bucket sets per group (Horner length); windows = sets * tables
  int gsets = 0;         // groups * sets
  int tables = 0;
  uint32_t nbk = 0;      // buckets per set = 2^(c-1)   (digit magnitudes 1..2^(c-1))
  // two-level counting sort: a bucket index b = (p << fb) | f; pass A partitions by p, pass B sorts by f
  int pb = 0, fb = 0;    // partition bits / fine bits, pb + fb = c - 1
  uint32_t bins = 0;     // gsets << pb
  uint32_t chA = 0;      // points per pass-A workgroup
  uint32_t nblkA = 0;    // pass-A workgroups
  uint32_t L = 0;        // sorted entries per accumulate thread: upper bound (the kernels use the actual entry count)
  uint32_t Lfixed = 0;   // tuning override: a fixed slice length (0 = computed on the device)
  uint32_t slots = 0;    // resident k_accumulate thread slots (workgroups per CU x 256 x CUs)
  uint32_t nthreads = 0; // accumulate threads
  uint32_t tstride = 0;  // points per fixed-base table (tables > 1)
  size_t ws_bytes = 0;
};
MsmPlan msm_make_plan(int groups, const size_t* n, const size_t* offsets, int c, int sets, int tables, int num_cus, int acc_fill = 0,
                      int scalar_bits = 256);
Status glv_points(int curve, const void* d_pts, size_t n, void* d_out, hipStream_t stream);      // [P | phi(P)]: 2n points
Status glv_split(int curve, const void* d_scalars, size_t n, bool is_mont, void* d_out, hipStream_t stream);   // [k1 | k2]: 2n sign-and-magnitude words
inline MsmPlan msm_make_plan(size_t n, int c, int sets, int tables, int num_cus) {
  const size_t zero = 0;
  return msm_make_plan(1, &n, &zero, c, sets, tables, num_cus);
}
int msm_auto_window(size_t n);
bool msm_plan_feasible(int groups, int c, int sets);       // sets <= 0: one bucket set per window (no table)
// d_points: table (tables*tstride affine) or plain bases (tables == 1).  d_scalars[g]: gn[g] x 32 B device.
// d_out: groups x 96 B device (Jacobian).  Enqueues on `stream`; no synchronisation.
// ev (optional): 4 events recorded at start / before accumulate / after accumulate / end.
// ext_bucket_acc (optional): the bucket accumulators of this plan's key range inside a job's shared array; the
// run then stops after the fix-up and msm_tail reduces all groups of the job at once.
Status msm_run(int curve, const MsmPlan& plan, const void* d_points, const void* const* d_scalars, bool is_mont,
               void* ws, void* d_out, hipStream_t stream, hipEvent_t* ev = nullptr, void* ext_bucket_acc = nullptr,
               hipEvent_t acc_gate = nullptr, int prio = 3);
size_t msm_tail_ws_bytes(int groups, int sets, uint32_t nbk);
Status msm_tail(int curve, int c, int sets, int groups, uint32_t nbk, void* tail_ws, void* d_out, hipStream_t stream, int prio = 3);
Status bases_generate(int curve, int family, uint64_t seed, size_t start, size_t n, void* d_pts, hipStream_t stream);
// msm_direct.hip: the digit table of generators [first, first + nslots) into slots [slot0, ...) of d_digits, and the
// direct sum over it (groups x 96 B Jacobian to d_out; ws: direct_ws_bytes)
int direct_windows(int c);
Status digits_build(int curve, const void* d_pts, size_t first, size_t nslots, size_t slot0, int c, void* d_digits, hipStream_t stream);
size_t direct_ws_bytes(int groups, const size_t* n, int c, int num_cus);
Status msm_direct_run(int curve, int groups, const size_t* n, const size_t* slot0, const void* const* d_scalars, bool is_mont,
                      int c, int num_cus, const void* d_digits, void* ws, void* d_out, uint32_t* arrived, hipStream_t stream);
Status bases_generate_label(int curve, const uint8_t* label, size_t len, size_t start, size_t n, void* d_pts, hipStream_t stream);
Status point_sum(int curve, const void* d_jac, size_t n, void* d_out, hipStream_t stream);
Status bases_validate(int curve, const void* d_pts, size_t n, uint32_t* d_flags, hipStream_t stream);   // d_flags: 2 words
Status bases_precompute(int curve, const void* d_pts, size_t n, int c, int sets, int tables, void* d_table,
                        hipStream_t stream);
// the even square root of n elements (d_ok[i] = 0 and a zero for a non-residue), and n points from their 32-byte wire
// encoding (d_ok[i] = 0 and a zeroed point for bytes that decode to none): every lane runs the same number of products
Status fe_sqrt_vec(int field, const void* d_a, size_t n, void* d_out, uint8_t* d_ok, hipStream_t stream);
Status points_decompress(int curve, const uint8_t* d_enc, size_t n, void* d_out, uint8_t* d_ok, hipStream_t stream);
Status points_axpy(int curve, const void* d_a, const void* d_b, const void* d_s, int bits, size_t n, void* d_out, hipStream_t stream);

// ---- vecops.hip ------------------------------------------------------------------------
Status vec_axpy(int field, const void* a, const void* r, const void* b, size_t n, void* out, hipStream_t s);
Status vec_cross_term(int field, const void* az1, const void* bz1, const void* cz1, const void* az2,
                      const void* bz2, const void* cz2, const void* u1, size_t n, void* T, hipStream_t s);
// two relaxed instances: u1, u2 and r are HOST elements whose values travel as kernel arguments; the fold is in place on the index-1 vectors
Status vec_cross_term_relaxed(int field, const void* az1, const void* bz1, const void* cz1, const vdf_fe* u1, const void* az2,
                              const void* bz2, const void* cz2, const vdf_fe* u2, size_t n, void* T, hipStream_t s);
Status vec_fold_relaxed(int field, const vdf_fe* r, size_t n, void* az1, void* bz1, void* cz1, void* e1, const void* az2,
                        const void* bz2, const void* cz2, const void* e2, const void* T, hipStream_t s);
Status vec_minroot_witness(int field, const void* trace_xy, const void* i0, uint64_t t, void* W, hipStream_t s);
Status vec_spmv_long(int field, const uint32_t* const rowptr[3], const uint32_t* const col[3], const uint32_t* const coef[3],
                     const void* dict, const void* z, const uint32_t* long_rows, size_t n_long, void* const out[3], hipStream_t s);
Status vec_spmv(int field, const uint32_t* rowptr, const uint32_t* col, const uint32_t* coef, const void* dict,
                const void* z, size_t rows, void* out, hipStream_t s);
// fused step kernels; vdf_fe* arguments are HOST pointers whose values travel as kernel arguments
Status vec_step_segment(int field, const void* trace_xy, uint64_t t, const vdf_fe* i0, int per, void* out, void* packed,
                        const vdf_fe* i_in, hipStream_t s);
// the forward circuit's variables for `lanes` traces lane_stride entries apart, lane-major into out (one launch; i_end: `lanes` host elements)
Status vec_forward_segment_lanes(int field, const void* trace_xy, size_t lane_stride, uint64_t t, size_t lanes, const vdf_fe* i_end, void* out,
                                 hipStream_t s);
// rounds.hip: a recorded round run over t repetitions (every index of the tape is checked before the launch; inv: host)
Status vec_round_tape(int field, const vdf_round_tape* tape, uint64_t t, const vdf_fe* inv, const void* advice, void* out, hipStream_t s);
Status vec_round_tape_lanes(int field, const vdf_round_tape* tape, uint64_t t, size_t lanes, const vdf_fe* inv, const void* advice,
                            size_t lane_stride, void* out, hipStream_t s);
Status vec_round_tape_walk_lanes(int field, const vdf_round_tape* tape, size_t lanes, const vdf_fe* inv, void* entries, size_t n,
                                 uint64_t rounds, void* trace, size_t walk_stride, size_t top, size_t group, size_t group_stride,
                                 const uint64_t* j_base, uint64_t j_group_step, int heads, const void* expect, int32_t* ok, hipStream_t s);
Status vec_round_tape_walk(int field, const vdf_round_tape* tape, const vdf_fe* inv, void* entries, size_t n, uint64_t rounds, void* trace,
                           size_t walk_stride, size_t top, size_t group, size_t group_stride, uint64_t j_base, uint64_t j_group_step,
                           int heads, const void* expect, int32_t* ok, hipStream_t s);
Status vec_round_tape_forward_walk(int field, const vdf_round_tape* tape, const vdf_fe* inv, void* entries, size_t n, uint64_t rounds,
                                   void* checkpoints, uint64_t every, size_t cp_stride, void* trace, size_t walk_stride, uint64_t base,
                                   uint64_t j_base, uint64_t j_walk_step, hipStream_t s);
Status vec_round_tape_rebuild_lanes(int field, const vdf_round_tape* tape, size_t lanes, const vdf_fe* inv, void* entries, size_t n,
                                    uint64_t rounds, void* trace, size_t walk_stride, uint64_t base, size_t group, size_t group_stride,
                                    const uint64_t* j_base, uint64_t j_group_step, int heads, const void* expect, int32_t* ok, hipStream_t s);
// launch_bound: the rounds a launch runs when the caller names no number (tape_launch.h forward_launch_bound)
Status round_tape_forward_max_rounds(const vdf_round_tape* tape, const vdf_fe* inv, uint64_t* max_rounds, uint64_t* launch_bound);
// The operands every cross-term launcher shares: the fresh z2, the running A z1, B z1, C z1 and u1 (host memory: it travels as a
// kernel argument), and what is written -- the fresh A z2, B z2, C z2 and T.  Host-side only: it ends at the launch line, where the
// kernels keep their own __restrict__ pointers.
struct CrossOperands { const void* z2; const void* abc1[3]; const vdf_fe* u1; void* abc2[3]; void* T; };
// rounds.hip: the cross term of periodic rows (vdf_hip.h vdf_periodic_rows; every index is checked before the launch)
Status vec_nifs_cross_periodic(int field, const vdf_periodic_rows* rows, uint64_t j_first, uint64_t reps, size_t seg_begin, size_t row0,
                               size_t num_cols, size_t num_cons, const CrossOperands& o, hipStream_t s);
Status vec_step_z(int field, const void* trace_xy, uint64_t t, const vdf_fe z_in[3], const vdf_fe* i0, const vdf_fe* u,
                  const vdf_fe X[6], void* z, void* packed, hipStream_t s);
Status vec_nifs_cross(int field, const uint32_t* const rowptr[3], const uint32_t* const col[3],
                      const uint32_t* const coef[3], const void* dict, const CrossOperands& o, size_t rows, size_t skip_begin,
                      size_t skip_len, const uint32_t* long_rowlist, size_t n_long_rows, double alg_bytes, hipStream_t s);
int nifs_cross_lanes(size_t rows);                       // lanes per row vec_nifs_cross picks for a launch over `rows` rows
Status vec_nifs_cross_minroot(int field, int per, uint64_t t, size_t seg_begin, size_t one_col, size_t row0, const CrossOperands& o,
                              hipStream_t s);
Status vec_nifs_cross_minroot_forward_lanes(int field, uint64_t t, size_t lanes, size_t seg_begin, size_t one_col, size_t row0,
                                            const CrossOperands& o, hipStream_t s);
// folded: o.abc1 again, as the pointers this variant alone WRITES through (the running rows, folded in place); r: host memory
Status vec_nifs_cross_minroot_fold(int field, int per, uint64_t t, size_t seg_begin, size_t one_col, size_t row0, const vdf_fe* r,
                                   void* const folded[3], void* e1, const void* tprev, const CrossOperands& o, hipStream_t s);
Status vec_fold_many(int field, const vdf_fe* r, int k, void* const acc[], const void* const add[], const size_t n[],
                     hipStream_t s);
// random linear combinations of many instances (vdf_lincomb_u128, vdf_relaxed_residual_batch): w and rho plain integers below
// 2^128, u Montgomery, all on the host; the residual's instances packed (residual_pack, residual_item_bytes() each) into a block
// the kernel reads from device memory
constexpr int LINCOMB_MAX = 64;                          // vectors of one vdf_lincomb_u128
constexpr int RESIDUAL_BATCH_MAX = 64;                   // instances of one vdf_relaxed_residual_batch
Status vec_lincomb_u128(int field, int count, const void* const v[], const size_t n[], const vdf_fe w[], size_t n_out, void* out,
                        hipStream_t s);
size_t residual_item_bytes();
void residual_pack(int count, const void* const z[], const void* const E[], const vdf_fe u[], const vdf_fe rho[], void* block);
Status vec_relaxed_residual_batch(int field, const uint32_t* const rowptr[3], const uint32_t* const col[3], const uint32_t* const coef[3],
                                  const void* dict, const void* block, int count, size_t rows, const uint32_t* long_rowlist,
                                  size_t n_long_rows, void* out, double alg_bytes, hipStream_t s);
// multi-point sparse evaluation (vdf_sparse_eval_multi): the instances (two device vectors, rho Montgomery; rho^2 made here)
// packed into a block the kernel reads from device memory; partials: sparse_eval_workgroups() x count elements of scratch
constexpr int SPARSE_EVAL_MAX = VDF_SPARSE_EVAL_MAX;     // instances of one vdf_sparse_eval_multi
size_t sparse_eval_item_bytes();
size_t sparse_eval_workgroups(size_t rows, size_t n_long_rows);
Status sparse_eval_pack(int field, int count, const void* const ex[], const void* const ey[], const vdf_fe rho[], void* block);
Status vec_sparse_eval_multi(int field, const uint32_t* const rowptr[3], const uint32_t* const col[3], const uint32_t* const coef[3],
                             const void* dict, const void* block, int count, size_t rows, size_t col_split, size_t col_hi_base,
                             const uint32_t* long_rowlist, size_t n_long_rows, void* partials, void* d_out, double alg_bytes,
                             hipStream_t s);
Status vec_mul(int field, const void* a, const void* b, size_t n, void* out, hipStream_t s);
Status vec_any_nonzero(const void* v, size_t n, uint32_t* d_flag, hipStream_t s);     // *d_flag = 1 iff some element is non-zero
Status vec_unsat_rows(int field, const void* a, const void* b, const void* c, size_t n, void* d_res, hipStream_t s);   // d_res[0] = rows with a b != c, d_res[1] = the first
Status vec_to_mont(int field, const void* a, size_t n, void* out, hipStream_t s);
Status vec_from_mont(int field, const void* a, size_t n, void* out, hipStream_t s);
Status vec_mul_chain(int field, const void* a, size_t n, int iters, void* out, hipStream_t s);
// out[i] = the family-0 random oracle of message i (n messages of len elements, message-major); rc: the 88 round constants
Status ro_hash_batch(int field, uint64_t tag, const void* d_rc, const void* d_xs, size_t len, size_t n, int bits, void* d_out, hipStream_t s);
// the shape refusals of a family-1 block, in the order width, full_rounds, partial_rounds (the ranges vdf_nova's ro_instance accepts)
Status ro_block_shape(int width, int full_rounds, int partial_rounds);
// out[i] = the family-1 random oracle of message i, one message per 32 lanes; rc: (full + partial) x width round constants
// (round-major), mds: width x width (row-major), both in Montgomery form
Status ro_hash_batch_block(int field, uint64_t tag, int width, int full_rounds, int partial_rounds, const void* d_rc, const void* d_mds,
                           const void* d_xs, size_t len, size_t n, int bits, void* d_out, hipStream_t s);
Status vec_clock_probe(int iters, int workgroups, unsigned long long* d_out3, hipStream_t s);   // d_out3 zeroed by the caller

// ---- minroot.hip -----------------------------------------------------------------------
// n walks of `rounds` inverse rounds in place over `states` (device, 96 B each); trace (device or null): walk w writes the
// (x, y) it stands on before round r to entry (w / group) * group_stride + (w % group) * walk_stride + top - r (group == 0: one group)
constexpr uint64_t MINROOT_WALK_MAX_ROUNDS = 1ull << 22;
Status minroot_inverse_walk(int field, void* states, size_t n, uint64_t rounds, void* trace, size_t walk_stride, size_t top,
                            size_t group, size_t group_stride, hipStream_t s);
// n walks of `rounds` FORWARD rounds (at most VDF_MINROOT_FORWARD_MAX_ROUNDS) in place over `states`; `base` = the rounds a walk has behind
// it: after round r walk w writes (x, y) to trace entry w * walk_stride + base + r + 1 (trace: device or null) and, when `every`
// divides g = base + r + 1, its state to checkpoints[w * cp_stride + g / every] (checkpoints: device or null)
Status minroot_forward_walk(int field, void* states, size_t n, uint64_t rounds, void* checkpoints, uint64_t every, size_t cp_stride,
                            void* trace, size_t walk_stride, uint64_t base, hipStream_t s);
Status minroot_states_match(const void* a, const void* b, size_t n, int* ok, hipStream_t s);      // ok[w] = (a[w] == b[w]), 96 B each
Status minroot_trace_heads(const void* states, size_t n, size_t state_stride, void* trace, size_t trace_stride, hipStream_t s);

// ---- snark.hip -------------------------------------------------------------------------
// vdf_fe* arguments are HOST pointers whose values travel as kernel arguments; void* are device vectors
Status snark_pair_table(int field, const vdf_fe* lo, const vdf_fe* hi, int k, void* out, hipStream_t s);
// the inner-product argument's coefficients (vdf_ipa_coefficients): the openings packed into a block of
// snark_ipa_block_bytes(count) bytes, which the kernel reads from device memory
size_t snark_ipa_block_bytes(int count);
void snark_ipa_pack(const vdf_ipa_opening* ops, int count, void* block);
Status snark_field_one(int field, vdf_fe* out);           // 1 in Montgomery form
Status snark_ipa_coefficients(int field, const void* block, int count, size_t n, void* out, hipStream_t s);
Status snark_fold_halves(int field, int k, void* const v[], const vdf_fe c_lo[], const vdf_fe c_hi[], size_t n, hipStream_t s);
size_t snark_reduce_scratch_bytes();
Status snark_reduce(int field, int kind, const void* const tables[], const vdf_fe* u, size_t n, void* scratch, void* out,
                    hipStream_t s);
Status snark_spmvt(int field, const uint32_t* colptr, const uint32_t* rows, const uint32_t* cm, const uint32_t* heavy,
                   size_t nheavy, size_t nbig, const void* dict, const void* eq, const vdf_fe* rho, size_t ncols, void* out, void* scratch,
                   hipStream_t s);
Status snark_ipa_scalars(int field, const void* a, const void* sv, size_t n, size_t nj, void* sL, void* sR, hipStream_t s);
Status snark_scale_pattern(int field, void* sv, size_t n, size_t nj, const vdf_fe* x_lo, const vdf_fe* x_hi, hipStream_t s);
// many instances at once: pointers and factors packed (snark_*_pack, snark_*_item_bytes() each) into a block the kernels read
// from device memory
constexpr int SNARK_FOLD_BATCH_MAX = 320;                 // vectors of one vdf_fold_halves_batch
constexpr int SNARK_REDUCE_BATCH_MAX = 512;               // instances of one vdf_reduce_batch (their partials fill the reduction scratch)
constexpr int SPMVT_BATCH = 4;                            // instances per launch of k_spmvt_batch (one accumulator each per lane)
size_t snark_reduce_item_bytes();
size_t snark_fold_item_bytes();
size_t snark_spmvt_item_bytes();
void snark_reduce_pack(int kind, int count, const void* const tables[], const vdf_fe* u, void* block);
void snark_fold_pack(int k, void* const v[], const vdf_fe c_lo[], const vdf_fe c_hi[], void* block);
void snark_spmvt_pack(int count, const void* const eq[], const vdf_fe rho[], void* const out[], void* block);
Status snark_reduce_batch(int field, int kind, const void* block, int count, size_t n, void* scratch, void* out, hipStream_t s);
Status snark_fold_halves_batch(int field, const void* block, int k, size_t n, hipStream_t s);
Status snark_spmvt_batch(int field, const uint32_t* colptr, const uint32_t* rows, const uint32_t* cm, const uint32_t* heavy,
                         size_t nheavy, size_t nbig, const void* dict, const void* block, int count, size_t ncols, void* scratch,
                         hipStream_t s);

}  // namespace vdf
