// Shared declarations of the translation units of libvdf_nova.so (minroot_host.cpp, r1cs.cpp, nova_host.cpp, trace_walks.cpp, circuits_host.cpp,
// custom_chain_host.cpp, compress_host.cpp, aggregate_host.cpp, wire_host.cpp): error plumbing, the two sides of the curve cycle, the handle structs.
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <mutex>
#include <vector>
#include "../../../include/vdf_nova.h"
#include "host_math.hpp"
#include "r1cs.hpp"
#include "rounds.hpp"
#include "trace_walks.hpp"

namespace vdfnova {
using namespace vdfhost;

int fail(int code, const std::string& msg);          // records the message for vdf_nova_last_error, returns code
// no C++ exception crosses the C ABI: an entry point that allocates or synthesises runs its body through this
template <class F>
inline int nova_guard(F&& body) {
  try { return body(); }
  catch (const std::bad_alloc&) { return fail(VDF_ERR_OOM, "host allocation failed"); }
  catch (const std::exception& ex) { return fail(VDF_ERR_DEVICE, ex.what()); }
  catch (...) { return fail(VDF_ERR_DEVICE, "unknown failure"); }
}
#define HIPCALL(ctx, expr)                                                          \
  do {                                                                              \
    int rc__ = (expr);                                                              \
    if (rc__ != VDF_OK) return ::vdfnova::fail(rc__, std::string(#expr) + ": " + vdf_last_error(ctx)); \
  } while (0)

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- MinRoot (minroot_host.cpp) -------------------------------------------------------------------------
struct St { Fe x, y, i; };
inline St load_state(const vdf_state* s) { St r; memcpy(&r, s, sizeof(St)); return r; }
inline void store_state(vdf_state* o, const St& s) { memcpy(o, &s, sizeof(St)); }
inline bool valid_field(int f) { return f == VDF_FIELD_FP || f == VDF_FIELD_FQ; }
inline bool valid_mode(int m) { return m >= 0 && m <= 3; }

// ---- Nova (nova_host.cpp) ---------------------------------------------------------------------------------
constexpr int NUM_IO = AUG_IO;             // public IO of an augmented circuit
constexpr uint64_t GENS_SEED = 0x4e6f7661; // "Nova": label of the generator families
constexpr int PRIMARY = 0, SECONDARY = 1;  // G1 / G2, src/nova/proof.rs:26-27: Pallas / Vesta when the parameters' field is Fq, Vesta / Pallas when it is Fp

// One side of the cycle: an augmented circuit over F (the scalar field of `curve`), its R1CS shape and the Pedersen
// generators its witnesses are committed under -- everything the folding, the satisfiability check and the
// compression argument need to know about "the instance's side".
// Scratch vectors of the compression SNARK, one block per side, kept by the parameter set from one call to the next (twelve
// device allocations and as many frees per vdf_nova_compress were 0.6 ms of its 27)
struct Arena { void* p = nullptr; size_t cap = 0; };
struct Side {
  int side = 0, field = 0, curve = 0;
  const Field* F = nullptr;                // scalars of this side's instances (= the circuit's field)
  const Field* Fb = nullptr;               // coordinates of this side's commitments
  vdf_ctx* ctx = nullptr;
  Arena* arena = nullptr;                  // the parameter set's scratch block for this side (compress / verify_compressed)
  vdf_ctx* ctx_b = nullptr;                // compress only (a copy of the side made for one call): a second queue for the E opening
  size_t num_cons = 0, num_vars = 0, ncols = 0, nnz3 = 0, num_gens = 0;
  vdf_shape* shape = nullptr;
  vdf_bases* gens = nullptr;
  Aff gen_u;                               // the extra generator of the inner-product arguments: number num_gens of the family
  void* d_zero = nullptr;                  // num_cons zero elements (satisfiability residual)
  uint8_t digest[32];                      // the parameters' digest (same on both sides; bound into the argument's transcript)
};

// instance of one side; u and X in Montgomery form of that side's own field
struct Inst { Aff comm_W, comm_E; Fe u; Fe X[NUM_IO]; };
RelaxedInst to_relaxed(const Inst& in, const Field& own);
// relaxed satisfiability of (inst, z = [W | u | X], E) on `sd`: commitments open and A z o B z = u C z + E
int check_sat(const Side& sd, const Inst& in, const void* d_z, const void* d_E, void* d_scratch_abc[3], void* d_scratch_T, bool* ok);
// sum_j sc[j] pts[j] over a few host points, Montgomery scalars (compress_host.cpp): enqueued on sd.ctx, *out ready after a sync
int msm_points(const Side& sd, const std::vector<Aff>& pts, const std::vector<Fe>& sc, vdf_jac* out);
// Deferred satisfiability checks of many instances of one side, combined with 128-bit weights the caller draws (nova_host.cpp,
// vdf_nova_verify_batch).  Opening: a vector committed to under the side's generators, its commitment and its weight (a plain
// integer below 2^128).  Residual: z = [W | u | X], E (null: zero), u, and its weight.
struct OpeningTerm { const void* d_v; size_t n; Aff comm; Fe w; };
struct ResidualTerm { const void* d_z; const void* d_E; Fe u; Fe w; };
// MSM(G, sum_j w_j v_j) == sum_j w_j C_j: vdf_lincomb_u128 in groups of 64 into d_scratch (max n elements), one MSM over the
// generators, one over the commitments
int check_openings_combined(const Side& sd, const std::vector<OpeningTerm>& terms, void* d_scratch, bool* ok);
// sum_j w_j (A z_j o B z_j - u_j C z_j - E_j) == 0: vdf_relaxed_residual_batch in groups of 64 into d_scratch (num_cons
// elements), each group tested for zero
int check_residuals_combined(const Side& sd, const std::vector<ResidualTerm>& terms, void* d_scratch, bool* ok);

}  // namespace vdfnova

using vdfhost::Aff; using vdfhost::Fe;
using vdfnova::NUM_IO;

struct vdf_pp {
  vdf_ctx* ctx = nullptr;
  uint64_t t = 0;
  int circuit_kind = 0, gens_family = 0;
  int field = VDF_FIELD_FQ;                // the orientation: the primary circuit's field, the VDF's (s[0].field; s[1] has the other one)
  vdfnova::Side s[2];
  uint8_t digest[32];                      // 250-bit little-endian integer
  Fe params[2];                            // the digest as an element of each side's field
  // variables of the primary witness that the GPU fills from the forward trace (the MinRoot rounds): [seg_begin, seg_begin + seg_len)
  size_t seg_begin = 0, seg_len = 0;
  // a custom circuit's vdf_cs_repeat as its shape synthesis recorded it (the body, t, where its variables begin): every
  // prove_step's own recording is compared with it; [seg_begin, seg_begin + seg_len) are its variables
  vdfnova::RepeatState round;
  void* d_round_table = nullptr;                   // the device copy of round.rec.table (vdf_cs_tab), null without one
  // ... and the rows of its repetitions as a periodic description, when they are one (detect_periodic_rows, checked against every
  // triple when the parameters were made); periodic_on: tuning.periodic_rows lets the prover use it (vdf_nova_pp_stencil == 7)
  vdfnova::PeriodicRows periodic;
  bool periodic_on = false;
  // constraints of the primary shape that read nothing of a fresh witness but that segment (and the constant): their
  // share of a step's cross term and of its commitment is made ahead of the rest, [ahead_row, ahead_row + ahead_rows)
  size_t ahead_row = 0, ahead_rows = 0;
  // the column of z_in[0] in the primary witness: where synthesize_augmented allocates the step circuit's `arity` inputs.  A built-in
  // kind's sit right in front of the segment (seg_begin - arity); a custom circuit may allocate variables of its own in between
  size_t zin_begin = 0;
  int stencil_per = 0;           // 5 / 6 (VDF_STENCIL_FORWARD / _LANES): the forward circuit's stencil, of one lane / of more -- one kernel
                                 // (vdf_nifs_cross_term_minroot_forward_lanes), the code only says how many lanes it runs;
                                 // 3 / 4: the early rows are the built-in MinRoot stencil with that many variables per round, checked against
                                 // the shape at public_params -- their cross term needs no sparse matrix (vdf_nifs_cross_term_minroot); 0: generic rows
  int ahead_mode = 2;            // when they run: 2 = from the start of the step, beside the secondary side's NIFS; 1 = after it (tuning)
  size_t arity = 3;                        // of the primary step circuit (z0, zi)
  size_t lanes = 1;                        // the forward kinds: evaluations advanced per step (arity = 3 lanes; VDF_CIRCUIT_MINROOT_FORWARD is the
                                           // circuit of one lane, and so is _LANES with lanes = 1); 1 for every other kind
  // the reference's step circuit only: generators of the packed commitment to the MinRoot rounds (3t + 4 points derived from
  // the 4t + 1 of the segment: vdf_hip.h vdf_minroot_step_segment_packed), with a fixed-base table of their own
  vdf_bases* seg_gens = nullptr;
  const vdfnova::RoInstance* ro = nullptr;  // the random oracle's parameter block (covered by the digest); never null once the set is made
  vdf_ctx* aux_ctx = nullptr;              // a second queue of the same device for compress (the secondary side's argument runs beside the
                                           // primary's, as nova-snark's CompressedSNARK::prove does); created on first use
  vdfnova::Arena arena[2];                 // compress / verify_compressed scratch, per side (freed with the set)
  vdf_ctx* aux_ctx2 = nullptr;             // ... and a third for the primary side's second opening (compress_host.cpp ipa_prove_two_queues)
  std::mutex aux_mu;                       // ... one compression at a time uses it: concurrent vdf_nova_compress calls under ONE parameter
                                           // set take turns at the arguments (calls under different sets do not meet)
  vdf_nova_tuning tune;                    // the tuning this set was made with, and that its prover runs with
  // vdf_nova_verify_compressed_batch: 0 = every replay evaluates its own M(r_x, r_y); n = 1..64: all of a side's by passes over the
  // shape of at most n points each (vdf_nova_pp_set_verify_multi; initial value: VDF_NOVA_VERIFY_MULTI, else verify_multi_default)
  std::atomic<int> verify_multi{0};
  std::atomic<uint64_t> verify_multi_stats[3] = {{0}, {0}, {0}};      // launches, points evaluated, points whose comparison failed
  // vdf_nova_verify_aggregate_device: 0 = an aggregate's per-entry Poseidon hashes are made on the host; n > 0: by three
  // vdf_ro_hash_batch launches when the aggregate holds at least n entries (vdf_nova_pp_set_verify_ro_device; the default block only)
  std::atomic<int> verify_ro_device{0};
  std::atomic<uint64_t> verify_ro_stats[2] = {{0}, {0}};               // hashes made on the device, launches
  void* d_ro_rc[2] = {nullptr, nullptr};   // each field's 88 round constants on the device (index: VDF_FIELD_*), made on first use under ro_mu
  // the same choice for a set made under another block: by three vdf_ro_hash_batch_block launches (vdf_nova_pp_set_verify_ro_block_device)
  std::atomic<int> verify_ro_block_device{0};
  void* d_ro_block[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [field][rc, mds] of the set's own block, made on first use under ro_mu
  std::mutex ro_mu;
  double setup_ms[7] = {0, 0, 0, 0, 0, 0, 0};
  uint64_t digit_table_bytes[2] = {0, 0};  // HBM held by each side's digit table (vdf_nova_pp_memory)
  unsigned digit_tables_skipped = 0;       // bit s: side s asked for a digit table and went without (no room, refused window)
};

struct Circuit : TraceSlot { // InverseMinRootCircuit<G1>, src/nova/proof.rs:57-66, + the forward trace; its TraceSlot: that trace in HBM
                            // (vdf_nova_circuits_upload, vdf_nova_circuits_materialize)
  uint64_t inverse_exponent = 5;
  vdfnova::St result, input;
  uint64_t t = 0;
  std::vector<Fe> trace_xy;  // (x, y) of states 0..t: trace[0] = input, trace[t] = result
  // a circuit made from checkpoints (vdf_nova_circuits_from_checkpoints) holds no host trace: the step's states every `every`
  // rounds in forward order, cp[0] = input .. cp[t / every] = result; its d_trace is built by walks, and is what release lets go of
  uint64_t every = 0;
  std::vector<vdfnova::St> cp;
  // a step of a forward chain in L >= 1 lanes (vdf_nova_circuits_forward_begin: L = 1, vdf_nova_circuits_lanes_begin): these hold every
  // lane's states and are what the forward circuit reads; result / input above are lane 0's (vdf_proof::Ahead and the inverse
  // kinds, which leave these empty, read those).  trace_xy and the device trace are L traces back to back, t + 1 entries each,
  // and cp is L runs of t / every + 1 states
  std::vector<vdfnova::St> lane_result, lane_input;
};
// What the walks of a vdf_circuits are to TraceWalks (trace_walks.hpp): inverse MinRoot walks over vdf_state entries (circuits_host.cpp).
// The C ABI hands prove_step and prove_recursively the circuits const (the reference takes them by value), and both finish or start
// walks under them: `walk` is the one member a const handle may change, and what the walks decide about a trace is written into
// v[k] through the one cast there is (CircuitWalks::slot, by circuits_host.cpp's `written`).
struct CircuitWalks final : vdfnova::WalkOwner {
  const vdf_circuits* c;
  std::vector<vdfnova::St> from, to;       // where a pending job's walks start and must land, in the walks' order
  explicit CircuitWalks(const vdf_circuits* c) : WalkOwner("circuits'", "circuits"), c(c) {}
  TraceSlot& slot(size_t k) override;
  void shape(size_t first_step, vdfnova::WalkJob* j) override;
  void stage_walks(const vdfnova::WalkJob& j, const void** starts, const void** expects) override;
  void unstage() override;
  int setup(vdf_ctx* q, const vdfnova::WalkJob& j, const vdfnova::WalkScratch& s) override;
  int launch(vdf_ctx* q, const vdfnova::WalkJob& j, const vdfnova::WalkScratch& s, uint64_t rounds, uint64_t top, int last) override;
  int finish(vdf_ctx* q, const vdfnova::WalkJob& j, const vdfnova::WalkScratch& s) override;
  std::string missed(size_t k, size_t walk) override;
};
struct vdf_circuits {
  std::vector<Circuit> v;
  int field = VDF_FIELD_FQ;                // the chain's field: its evaluator, its counters, its push checks and its walks run over it
  bool checkpoints = false;                // made by vdf_nova_circuits_from_checkpoints (or grown by vdf_nova_circuits_push_checkpoints)
  // a forward chain (vdf_nova_circuits_forward_begin, vdf_nova_circuits_lanes_begin): circuits in the order of evaluation, appended
  // to while the chain grows; lane_end[l] is the state lane l of the next pushed step must start from
  bool forward = false;
  uint64_t forward_t = 0;
  size_t lanes = 1;                        // evaluations advanced per step (1: a single chain)
  std::vector<vdfnova::St> lane_end;       // a forward chain: where every lane stands
  vdfnova::St end;                         // ... lane 0's
  CircuitWalks walked{this};
  mutable vdfnova::TraceWalks walk{&walked};   // (walk.home: where the traces live)
};

// NovaVDFProof::Recursive = nova-snark RecursiveSNARK: running instance + witness on both sides, the last secondary
// instance unfolded, the step counter and both z_i.  Constant size in the number of steps.
struct SideState {
  vdfnova::Inst inst;        // running relaxed instance
  void* d_z = nullptr;       // [W | u | X]
  void* d_E = nullptr;
  void* d_abc[3] = {};       // A z, B z, C z of the running instance, folded along (linear in z)
  void* d_abc2[3] = {};      // the fresh instance's
  void* d_T = nullptr;
  // The operands of a cross term of this running instance with a fresh z2, typed and ordered as every vdf_nifs_cross_term* of
  // include/vdf_hip.h takes them (CROSS_ARGS): z2, A z1, B z1, C z1, u1 | A z2, B z2, C z2, T
  struct Cross { const vdf_fe* z2; const vdf_fe* abc1[3]; const vdf_fe* u1; vdf_fe* abc2[3]; vdf_fe* T; };
  Cross cross(const void* d_z2) const {
    return {(const vdf_fe*)d_z2, {(const vdf_fe*)d_abc[0], (const vdf_fe*)d_abc[1], (const vdf_fe*)d_abc[2]}, (const vdf_fe*)&inst.u,
            {(vdf_fe*)d_abc2[0], (vdf_fe*)d_abc2[1], (vdf_fe*)d_abc2[2]}, (vdf_fe*)d_T};
  }
};
#define CROSS_ARGS(c) (c).z2, (c).abc1[0], (c).abc1[1], (c).abc1[2], (c).u1, (c).abc2[0], (c).abc2[1], (c).abc2[2], (c).T
// A z2, B z2, C z2 and T of EVERY row of side S through its sparse matrices, enqueued on q (nova_host.cpp has the other entry points)
inline int cross_all(vdf_ctx* q, const vdfnova::Side& S, const SideState& st, const void* d_z2) {
  const SideState::Cross c = st.cross(d_z2);
  HIPCALL(q, vdf_nifs_cross_term(q, S.shape, CROSS_ARGS(c)));
  return VDF_OK;
}
struct vdf_proof {
  vdf_pp* pp = nullptr;
  size_t i = 0;
  std::vector<Fe> zi[2], z0[2];
  SideState r[2];
  // fresh secondary instance (u = 1, E = 0)
  vdfnova::Inst l2;
  void* d_l2z = nullptr;
  bool l2_committed = false;
  // The NIFS of the last secondary instance (cross term, commit(w2), commit(T2)) needs nothing of the next step: prove_step
  // launches it on its way out, the next prove_step only waits for it.  NONE: not launched / results used or overwritten;
  // INFLIGHT: on the queue, results going to h_pts[RING], h_pts[RING + 1]; DONE: collected (comm_T2 in nifs2_T, A z, B z,
  // C z and T of the fresh instance still in the secondary side's scratch vectors)
  enum { NIFS2_NONE = 0, NIFS2_INFLIGHT = 1, NIFS2_DONE = 2 };
  int nifs2 = NIFS2_NONE;
  Aff nifs2_T;
  // ... and so do the early rows of the NEXT step's cross term, when that step's rounds are already in their ring slot
  // (the lookahead): launched on the way out of a step too; valid for the step that finds this slot and circuit
  bool tahead_valid = false;
  bool poisoned = false;         // a fused fold was begun and the stencil that finishes it never reached its queue (a device failure): the running
                                 // instance is half folded and every later call on this proof is refused
  int tahead_slot = -1;
  size_t tahead_k = 0;
  const vdf_circuits* tahead_circuits = nullptr;
  const vdf_custom_chain* tahead_chain = nullptr;     // ... of a custom chain's step (tuning.custom_ahead = 2; tahead_circuits is null then)
  // fresh primary z: ring of slots, the MinRoot segment of a later step is filled (and committed) ahead of time on ctx2
  static constexpr int DEPTH = 1, RING = DEPTH + 2;
  vdf_ctx* ctx2[DEPTH] = {};
  vdf_ctx* ctx3 = nullptr;       // the early rows of a step's cross term and their commitment: a queue of their own, so that
                                 // they start with the step and not behind the previous lookahead's commitment
  void* d_z2s[RING] = {};
  void* d_traces[DEPTH] = {};
  void* d_packed[DEPTH] = {};    // scalars of the packed commitment (the reference's circuit), one buffer per lookahead queue
  int slot = 0;
  struct Ahead { vdfnova::St result, input; int slot; };
  const vdf_circuits* ahead_circuits = nullptr;
  size_t ahead_k = 0;
  std::vector<Ahead> ahead;
  // The lookahead of a custom chain (tuning.custom_ahead): the rounds of step k of `chain` are in ring slot `slot` (ahead[0] names it
  // too) and their commitment is on its way to h_pts[slot], made from the trace d_trace with the `inv` a probe synthesis captured.
  // The step that comes compares all of it with what its own vdf_cs_repeat sees (StepRun::lookahead_select, chain_primary_circuit).
  struct CustomAhead {
    bool valid = false;
    const vdf_custom_chain* chain = nullptr;
    size_t k = 0;
    const vdf_fe* d_trace = nullptr;
    size_t lane_stride = 0;
    std::vector<Fe> inv;
    int slot = -1;
  } cahead;
  uint64_t ahead_hits = 0, ahead_misses = 0, ahead_skipped = 0;     // vdf_nova_proof_ahead_stats
  Fe* h_zin = nullptr;           // pinned: the step circuit's input for the early rows of T
  vdf_jac* h_pts = nullptr;      // pinned result slots: [0, RING) segment commitments per ring slot, 4 for the batches, 1 for the early rows of T
  Fe* h_stage[2] = {};           // pinned staging of a host-synthesised witness, one per side
  // vdf_nova_proof_last_unsat: the last prove_step of THIS object left its fresh primary z in d_z2s[slot]; A z, B z, C z of it are
  // made again on request into these (allocated by the first request)
  bool stepped = false;
  void* d_unsat[3] = {};
  // the last step's by-products, for the parity tests
  vdf_nova_step_info last;
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace vdfnova {
const vdf_nova_tuning& default_tuning();   // defaults + the VDF_NOVA_* environment overrides, read once
int verify_multi_default();                // VDF_NOVA_VERIFY_MULTI (0..64) when set, else the shipped default (compress_host.cpp)
bool tuning_valid(const vdf_nova_tuning& t);
int alloc_proof_buffers(vdf_proof* p);
int finalize_l2(const vdf_proof* p);      // commits to the last secondary witness if that is still pending
std::unique_ptr<StepCircuit> make_primary_circuit(const vdf_pp* pp, const Circuit* c, bool device_rounds);
// probe: the synthesis is the extra one of tuning.custom_ahead (vdf_cs_is_probe; its vdf_cs_repeat touches neither advice nor cs)
std::unique_ptr<StepCircuit> make_custom_circuit(const vdf_step_circuit* c, vdf_ctx* ctx = nullptr, const vdf_fe* step_advice = nullptr,
                                                 size_t step_advice_elems = 0, bool probe = false);
// ---- the circuits as the drivers of nova_host.cpp reach them (circuits_host.cpp) --------------------------------------------
inline void eval_step(int field, int mode, uint64_t t, St* state, Fe* trace_xy) {   // t rounds from *state: the trace [2 (t + 1)], *state = the result
  vdf_state in, res;
  store_state(&in, *state);
  vdf_minroot_eval(field, mode, &in, t, &res, (vdf_fe*)trace_xy);
  *state = load_state(&res);
}
inline bool needs_walk(const Circuit& c) { return !c.d_trace && !c.cp.empty(); }   // not resident and has checkpoints
// checkpoint circuits: finish the pending walks if they cover circuit k and say whether its trace is there;
// enqueue the share of the pending walks that keeps them ahead of a prover about to prove circuit k
int circuits_need(const vdf_circuits* c, size_t k);
int circuits_pump(const vdf_circuits* c, size_t k);
// vdf_nova_circuits_materialize for the windowed prover, which is handed the circuits const
int circuits_materialize(vdf_ctx* ctx, const vdf_circuits* c, size_t first, size_t count, int wait, int* bad);

// ---- a custom circuit's chain as the drivers of nova_host.cpp reach it (custom_chain_host.cpp) ------------------------------
// what the prover must know of a chain before it hands a step's trace to a circuit
struct ChainInfo { int field; uint64_t t; size_t n_adv, steps; vdf_ctx* ctx; size_t lanes; };
ChainInfo chain_info(const vdf_custom_chain* c);
TraceWalks& chain_walks(vdf_custom_chain* c);
// finish the pending walks if they cover step k and hand out its device trace (refused when there is none); enqueue the share
// of the pending walks that keeps them ahead of a prover about to prove step k
int chain_need(vdf_custom_chain* c, size_t k, const vdf_fe** d_trace);
int chain_pump(vdf_custom_chain* c, size_t k);
// step k's device trace when it is RESOLVED: resident, and no pending walks cover it (they are finished -- the walk queue has been
// synchronised by the host -- and every one of them landed on its checkpoint); null otherwise.  Never waits.
const vdf_fe* chain_ready(const vdf_custom_chain* c, size_t k);

// ---- wire formats (wire_host.cpp; layout in include/vdf_nova.h) --------------------------------------------
constexpr char WIRE_MAGIC_SNARK[9] = "VDFSNK03";      // compressed proof
constexpr char WIRE_MAGIC_PROOF[9] = "VDFRSK02";      // running proof (checkpoint)
inline uint8_t* wire_put_fe(uint8_t* o, const Fe& v, const Field& F) { const Fe c = from_mont(v, F); memcpy(o, c.l, 32); return o + 32; }
inline bool wire_get_fe(const uint8_t* i, const Field& F, Fe* v) {
  Fe c;
  memcpy(c.l, i, 32);
  if (geq(c.l, F.m)) return false;
  *v = to_mont(c, F);
  return true;
}
// an instance on the wire: commitment(s) as 32-byte points, then (u and) X; a strict instance has no comm_E and u = 1
inline uint8_t* put_inst(uint8_t* o, const Inst& in, const Side& sd, bool relaxed) {
  pt_compress(in.comm_W, *sd.Fb, o); o += 32;
  if (relaxed) { pt_compress(in.comm_E, *sd.Fb, o); o += 32; o = wire_put_fe(o, in.u, *sd.F); }
  for (int k = 0; k < NUM_IO; ++k) o = wire_put_fe(o, in.X[k], *sd.F);
  return o;
}
// point(enc, sd, dst): what becomes of a 32-byte point encoding of side sd -- decoded on the spot (get_inst below), or noted for
// a batch that decodes every entry's points in one launch per curve (compress_host.cpp)
template <class PointFn>
inline const uint8_t* get_inst_points(const uint8_t* i, Inst* in, const Side& sd, bool relaxed, bool* canonical, PointFn&& point) {
  point(i, sd, &in->comm_W); i += 32;
  if (relaxed) {
    point(i, sd, &in->comm_E); i += 32;
    *canonical &= wire_get_fe(i, *sd.F, &in->u); i += 32;
  } else {
    memset(&in->comm_E, 0, sizeof(Aff));
    in->u = one(*sd.F);
  }
  for (int k = 0; k < NUM_IO; ++k) { *canonical &= wire_get_fe(i, *sd.F, &in->X[k]); i += 32; }
  return i;
}
inline const uint8_t* get_inst(const uint8_t* i, Inst* in, const Side& sd, bool relaxed, bool* canonical, bool* on_curve) {
  return get_inst_points(i, in, sd, relaxed, canonical,
                         [&](const uint8_t* enc, const Side& s, Aff* dst) { *on_curve &= pt_decompress(enc, *s.Fb, dst); });
}
constexpr size_t INST_WIRE_RELAXED = 32 * 5, INST_WIRE_STRICT = 32 * 3;
}  // namespace vdfnova

// ---- the compression argument as compress_host.cpp lends it to aggregate_host.cpp -------------------------------------------
namespace vdfnova {
// Protocol "vdf-spartan-v3", restated line by line by the test oracle (spartan.py: prove / verify): the transcript, the proof
// objects and the device scratch of compress_host.cpp.
struct Transcript {
  uint8_t state[32];
  explicit Transcript(const char* label) {
    Shake256 h;
    h.absorb("vdf-spartan-v3|", 15);
    h.absorb(label, strlen(label));
    h.squeeze(state, 32);
  }
  void absorb(const char* label, const void* data, size_t n) {
    Shake256 h;
    h.absorb(state, 32);
    h.absorb(label, strlen(label));
    h.absorb(":", 1);
    h.absorb(data, n);
    h.squeeze(state, 32);
  }
  void absorb_fe(const char* label, const Fe* v, size_t k, const Field& F) {
    std::vector<uint8_t> b(k * 32);
    for (size_t i = 0; i < k; ++i) { const Fe c = from_mont(v[i], F); memcpy(&b[i * 32], c.l, 32); }
    absorb(label, b.data(), b.size());
  }
  void absorb_pt(const char* label, const Aff* p, size_t k, const Field& F) {      // F: the points' coordinate field
    std::vector<uint8_t> b(k * 64, 0);
    for (size_t i = 0; i < k; ++i)
      if (!p[i].is_id()) {
        const Fe x = from_mont(p[i].x, F), y = from_mont(p[i].y, F);
        memcpy(&b[i * 64], x.l, 32); memcpy(&b[i * 64 + 32], y.l, 32);
      }
    absorb(label, b.data(), b.size());
  }
  // 128-bit challenge: raw = the integer, return = its Montgomery form in F
  Fe challenge(const char* label, const Field& F, uint64_t raw[4]) {
    Shake256 h;
    h.absorb(state, 32);
    h.absorb(label, strlen(label));
    h.absorb("?", 1);
    uint8_t out[48];
    h.squeeze(out, 48);
    memcpy(state, out + 16, 32);
    raw[0] = raw[1] = raw[2] = raw[3] = 0;
    memcpy(raw, out, 16);
    Fe r;
    memcpy(r.l, raw, 32);
    return to_mont(r, F);
  }
};

// The halving of an inner-product argument stops at IPA_STOP elements: the prover sends that vector instead of four more
// rounds (each a pair of MSMs over all generators for the prover; the verifier's one MSM is the same either way).
constexpr size_t IPA_STOP = 16;
inline size_t ipa_final(size_t n) { return n < IPA_STOP ? n : IPA_STOP; }
inline size_t ipa_rounds(size_t n) { size_t k = 0; for (size_t m = n; m > IPA_STOP; m >>= 1) ++k; return k; }
struct Ipa { std::vector<Aff> L, R; std::vector<Fe> a; };
struct Spartan {
  std::vector<std::array<Fe, 3>> outer;
  Fe claims[4];
  std::vector<std::array<Fe, 2>> inner;
  Fe w_eval;
  Ipa ipaW, ipaE;
};

struct Layout { size_t M, NW, Z; int s, l1; };
Layout layout_of(const Side& sd);

// device buffers released on scope exit
struct DevBufs {
  vdf_ctx* ctx;
  Arena* arena;                    // the side's block (kept by the parameter set), or none: every vector its own allocation
  size_t reserved = 0, used = 0;
  std::vector<void*> v;
  explicit DevBufs(vdf_ctx* c, Arena* a = nullptr) : ctx(c), arena(a) {}
  ~DevBufs() { for (void* p : v) vdf_dev_free(ctx, p); }
  // all vectors of a call at once: one allocation the first time (or when a larger call comes), one memset every time
  int reserve(size_t elems) {
    if (!arena) return VDF_OK;
    const size_t bytes = elems * 32;
    if (arena->cap < bytes) {
      if (arena->p) { vdf_ctx_sync(ctx); vdf_dev_free(ctx, arena->p); arena->p = nullptr; arena->cap = 0; }
      int rc = vdf_dev_alloc(ctx, bytes, &arena->p);
      if (rc != VDF_OK) return rc;
      arena->cap = bytes;
    }
    reserved = bytes; used = 0;
    return vdf_dev_memset(ctx, arena->p, 0, bytes);
  }
  int zeros(size_t elems, void** out) {
    if (arena && used + elems * 32 <= reserved) { *out = static_cast<char*>(arena->p) + used; used += elems * 32; return VDF_OK; }
    int rc = vdf_dev_alloc(ctx, elems * 32, out);
    if (rc != VDF_OK) return rc;
    v.push_back(*out);
    return vdf_dev_memset(ctx, *out, 0, elems * 32);
  }
};

// What is left of an opening's check once the transcript is replayed: with Q' = c gen_u (c the 128-bit challenge) and ab the
// sent vector against b's fold,
//   P + c (v - ab) gen_u + sum_j (x_j^2 L_j + x_j^-2 R_j) == MSM(G, coefficients)
// where the coefficients are vdf_ipa_coefficients' table of the rounds (lo = x^-1, hi = x) over the sent vector a.  Linear in
// the group: checks of many openings combine with random weights into one equation (vdf_nova_verify_compressed_batch).
struct IpaDeferred {
  size_t n = 0;
  int k = 0, log_m = 0;
  std::vector<Fe> xs, xis;         // the round challenges and their inverses
  std::vector<Aff> lr_pts;         // L_0, R_0, L_1, R_1, ...
  std::vector<Fe> lr_sc;           // x_0^2, x_0^-2, ...
  std::vector<Fe> a;               // the sent vector (2^log_m elements)
  Aff P;
  Fe v, ab;
  uint64_t q_raw[4];
};

// the statement and witness of one side's argument
struct ProveIn { Aff cW, cE; Fe u; const Fe* X; const void* d_z; const void* d_E; Spartan* out; };

void instance_bytes(Transcript& tr, const Side& sd, const Aff& cW, const Aff& cE, const Fe& u, const Fe* X);
// one opening's deferred check on its own (d_s: n device elements of scratch)
int ipa_check_one(const Side& sd, const IpaDeferred& d, void* d_s, bool* ok);
// the single verifier's replay of one side's argument: the host part, then M(r_x, r_y) on the device
int spartan_replay(const Side& sd, const Aff& cW, const Aff& cE, const Fe& u, const Fe* X, const Spartan& pf, IpaDeferred out[2], bool* ok);
// instance fold on the host: U + r u with the cross-term commitment T; the NIFS challenge the circuits recompute
Inst fold_instance(const Side& sd, const Inst& U, const Inst& u, const Aff& T, const uint64_t r[4]);
void fold_challenge(const vdf_pp* pp, const Inst& U2, const Inst& l2, const Aff& T2, uint64_t r[4]);
size_t spartan_wire_size(const Layout& L);
void spartan_resize(Spartan& p, const Layout& L);
size_t statement_wire(size_t arity);      // the statement part of "VDFSNK03" (and of every entry of "VDFAGG01")
}  // namespace vdfnova

struct vdf_snark {          // NovaVDFProof::Compressed, src/nova/proof.rs:54 = nova-snark CompressedSNARK
  vdfnova::Inst r_U1, r_U2, l_u2;    // running primary, running secondary BEFORE the last fold, the last secondary instance
  Aff T2;                   // cross-term commitment of that last fold
  vdfnova::Spartan sp[2];   // sp[0]: r_U1 is satisfiable; sp[1]: fold(r_U2, l_u2) is
  std::vector<Fe> zi1;      // z_i of the primary side (arity of its step circuit)
  Fe zi2[1];
  uint64_t t = 0;           // the public parameters it was made under (wire header)
  uint8_t digest[32];
  int field = VDF_FIELD_FQ; // ... and their orientation: the primary side's scalar field (what the encodings below reduce by)
};

namespace vdfnova {
// the statement of a compressed proof, and the last secondary instance folded into the running one (scratch d_fz / d_fE; *f2: the folded instance)
int compress_prelude(const vdf_proof* p, vdf_pp* pp, vdf_snark* s, void* d_fz, void* d_fE, Inst* f2);
// both sides' arguments of K statements (the caller holds pp->aux_mu)
int prove_both_sides(vdf_pp* pp, size_t K, const ProveIn* in1, const ProveIn* in2, Arena* arena1, Arena* arena2);
constexpr char WIRE_MAGIC_AGGREGATE[9] = "VDFAGG01";  // aggregate of compressed proofs (aggregate_host.cpp)
}  // namespace vdfnova
