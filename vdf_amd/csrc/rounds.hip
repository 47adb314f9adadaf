// Round tapes (include/vdf_hip.h vdf_round_tape): the variables of t uniform repetitions of a step-circuit round that the host
// layer recorded from a callback (libvdf_nova.so vdf_cs_repeat) -- the device side of the step-circuit seam
// (/root/reference/src/nova/proof.rs:79-153, trait StepCircuit) for rounds this library did not write itself.
//
// One thread per repetition, workgroups of one wavefront.  The tape travels in the kernel arguments, so every lane reads the same
// op through scalar loads and the branch on the opcode is uniform.  The value file is in LDS, not in registers: a slot number is
// a run-time value, and a private array indexed by one would live in scratch.  Layout [slot][half][lane] of 16-byte halves, so a
// wavefront's access to one half of one slot is 64 consecutive uint4 (1 KiB): conflict-free under ds_read_b128 / ds_write_b128's
// lane groups.  A lane only ever touches its own column: no barrier.  LDS per workgroup is n_slots x 2 KiB, chosen at launch --
// the slot allocation of the recorder (live ranges, linear scan) is what keeps occupancy up, not the length of the tape.
#include <cstring>
#include <type_traits>
#include "internal.h"
#include "fe.cuh"
#include "cross.cuh"
#include "tape_launch.h"
#include "periodic_rules.h"

namespace vdf {

struct TapeFe { uint32_t v[8]; };
struct TapeArgs {
  uint32_t n_ops, n_vars, n_adv, pad;
  uint32_t ops[VDF_TAPE_MAX_OPS];                   // op | dst << 8 | a << 16 | b << 24
  TapeFe consts[VDF_TAPE_MAX_CONSTS];
  TapeFe inv[VDF_TAPE_MAX_INV];
};
static_assert(sizeof(TapeArgs) + 32 <= 4096, "the tape travels in the kernel-argument segment");

template <class P> __device__ __forceinline__ Fe<P> tape_fe(const TapeFe& a) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = a.v[i];
  return r;
}
template <class P> __device__ __forceinline__ Fe<P> slot_load(const uint4* lds, uint32_t slot, uint32_t lane) {
  const uint4 lo = lds[(slot * 2) * 64 + lane], hi = lds[(slot * 2 + 1) * 64 + lane];
  Fe<P> r;
  r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
  r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
  return r;
}
template <class P> __device__ __forceinline__ void slot_store(uint4* lds, uint32_t slot, uint32_t lane, const Fe<P>& a) {
  lds[(slot * 2) * 64 + lane] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  lds[(slot * 2 + 1) * 64 + lane] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}

// ---- the interpreter: the ops of ONE round of a tape for one lane, the only statement of them on the device -------------------
// Seven kernels run tapes (the two round kernels, the two descending walks, the two forward walks, the ascending rebuild), and six
// more the tapes that hold a VDF_TAPE_TAB (k_*_tab, below); they differ in their setup and landing and in three ops, which a kernel hands over as its
// IO: where ADV reads (global advice, or the entry stood on in LDS),
// where INV reads (the kernel arguments from an offset, or slots of LDS) and where OUT writes (global variables, or the entry
// produced in LDS).  ADMIT: the ops beyond the base set that the kernel's launcher lets through (pack_tape's mode) -- an op that is
// not admitted has no case here, so a kernel pays in registers and code only for what it can meet.
// What every kernel relies on: the slot file is in LDS, a lane touching only its own column (no barrier); nothing private is
// indexed by a run-time value (slot numbers, columns and constant indices are scalars read from the arguments, and index LDS or the
// arguments, never a register array: that would be scratch); control is wave-uniform (the opcode, every trip count and every
// exponent bit come from the kernel arguments by scalar loads).  No index is checked here: tape_rules.h has checked them all.
//
// A NEW OP touches exactly: the op enum in include/vdf_hip.h; the rules in tape_rules.h; tape_round below; the host interpreter
// run_tape_round in host/rounds_host.cpp (a separate restatement: the GPU tests compare the two); the recorder's compile_round there.
// A NEW LAUNCH KIND touches exactly: a Kind in tape_launch.h with its slots and whatever it is refused for beyond the skeleton there
// (both libraries read the refusals from that header, never from here); its kernel and launcher below, which packs and launches;
// its index arithmetic restated in host/rounds_host.cpp (separately, unless it is shared through the header as the rebuild's is);
// its rows in tests/launch_rules_spec.py.
enum { TAPE_BASE = 0, TAPE_POW = 1, TAPE_POWC = 2 };      // ADMIT: the base ops; and VDF_TAPE_POW; and VDF_TAPE_POWC
constexpr int TAPE_NO_OP = 0x100;                         // the case label of an op that is not admitted: an opcode is one byte

// VDF_TAPE_TAB is admitted by a second parameter, TAB, a type: NoTab for every tape without one -- the kernels those tapes always
// launched, unchanged to the instruction -- and TabIO for a tape that holds a TAB, in kernels of their own (k_*_tab).  The table lies
// in device-readable memory, not in the kernel arguments: 1 MiB would not fit, and the row is a per-lane value (one repetition per
// lane, one walk per lane), which as an index into the arguments would send them to scratch.  So a TAB is a per-lane 32-byte global
// load from a scalar base at (row * cols + a) * 32, and its value goes into its slot of LDS like any other; control stays uniform.
// The row is exactly J mod rows: the round kernels take the remainder once per thread; a walk takes it once, before its rounds, and
// then steps it with J -- down from 0 to rows - 1, up from rows - 1 to 0 -- except where J itself wraps modulo 2^64, which no
// increment of the row follows when rows is no power of two: there (J = 2^64 - 1 after a step down, J = 0 after a step up: a
// compare of the counter, uniform or not it is two selects) the remainder is taken again.  Nothing here can index out of range:
// row < rows by construction, a < cols by tape_rules.h.
struct NoTab {};
struct TabArgs { const char* table; uint32_t rows, cols; };      // behind the existing arguments of a k_*_tab kernel
struct TabIO {
  const char* table;
  uint32_t rows, cols, row;
  __device__ __forceinline__ void at(uint64_t j) { row = (uint32_t)(j % rows); }
  __device__ __forceinline__ void down(uint64_t j) { row = j == ~0ull ? (uint32_t)(j % rows) : row == 0 ? rows - 1 : row - 1; }      // j: after the step
  __device__ __forceinline__ void up(uint64_t j) { row = j == 0 ? 0u : row + 1 == rows ? 0u : row + 1; }
  template <class P> __device__ __forceinline__ Fe<P> load(uint32_t a) const { return fe_load<P>(table + ((size_t)row * cols + a) * 32); }
};
__device__ __forceinline__ TabIO tab_io(const TabArgs& t) { return TabIO{t.table, t.rows, t.cols, 0}; }

// k_round_tape, k_round_tape_lanes: advice and variables in global memory, this launch's (lane's) invariants from tape.inv[inv0]
template <class P> struct RoundIO {
  const char* adv;
  char* out;
  uint32_t inv0;
  __device__ __forceinline__ Fe<P> load_adv(const TapeArgs& tape, const uint4*, uint32_t, uint32_t a, uint32_t b) const {
    return fe_load<P>(adv + (b * tape.n_adv + a) * 32);
  }
  __device__ __forceinline__ Fe<P> load_inv(const TapeArgs& tape, const uint4*, uint32_t, uint32_t a) const { return tape_fe<P>(tape.inv[inv0 + a]); }
  __device__ __forceinline__ void store_out(uint4*, uint32_t, uint32_t b, const Fe<P>& v) const { fe_store<P>(out + b * 32, v); }
};
// the walks: ADV is the entry stood on (the launcher admits one b only), OUT the entry produced, both slots of LDS behind the value
// file; INV_LDS: the invariants are slots too, from inv0 (k_tape_walk_lanes), else tape.inv as it is
template <class P, bool INV_LDS> struct WalkIO {
  uint32_t stand, prod, inv0;
  __device__ __forceinline__ Fe<P> load_adv(const TapeArgs&, const uint4* slots, uint32_t lane, uint32_t a, uint32_t) const {
    return slot_load<P>(slots, stand + a, lane);
  }
  __device__ __forceinline__ Fe<P> load_inv(const TapeArgs& tape, const uint4* slots, uint32_t lane, uint32_t a) const {
    if constexpr (INV_LDS) return slot_load<P>(slots, inv0 + a, lane);
    else return tape_fe<P>(tape.inv[a]);
  }
  __device__ __forceinline__ void store_out(uint4* slots, uint32_t lane, uint32_t b, const Fe<P>& v) const { slot_store<P>(slots, prod + b, lane, v); }
};

// tmp0: T[0] of a chain, the first of the n_tmp slots behind the two entries (ADMIT = TAPE_POWC only)
template <class P, int ADMIT, class IO, class TAB = NoTab>
__device__ __forceinline__ void tape_round(const TapeArgs& tape, uint4* slots, uint32_t lane, uint64_t j, const IO& io, uint32_t tmp0 = 0,
                                           const TAB& tab = TAB()) {
  constexpr bool HAS_TAB = !std::is_same<TAB, NoTab>::value;
#pragma unroll 1
  for (uint32_t i = 0; i < tape.n_ops; ++i) {
    const uint32_t x = tape.ops[i];
    const uint32_t op = x & 0xFF, dst = (x >> 8) & 0xFF, a = (x >> 16) & 0xFF, b = x >> 24;
    Fe<P> v;
    switch (op) {
      case VDF_TAPE_ADV: v = io.load_adv(tape, slots, lane, a, b); break;
      case VDF_TAPE_INV: v = io.load_inv(tape, slots, lane, a); break;
      case VDF_TAPE_J: v = fe_from_u64<P>(j); break;
      case VDF_TAPE_CONST: v = tape_fe<P>(tape.consts[a]); break;
      case VDF_TAPE_ADD: v = fe_add(slot_load<P>(slots, a, lane), slot_load<P>(slots, b, lane)); break;
      case VDF_TAPE_SUB: v = fe_sub(slot_load<P>(slots, a, lane), slot_load<P>(slots, b, lane)); break;
      case VDF_TAPE_MUL: {
        const Fe<P> y = slot_load<P>(slots, a, lane);
        v = a == b ? fe_sqr(y) : fe_mul(y, slot_load<P>(slots, b, lane));
        break;
      }
      case VDF_TAPE_SCALE: v = fe_mul(slot_load<P>(slots, a, lane), tape_fe<P>(tape.consts[b])); break;
      // left-to-right square-and-multiply from the exponent's top set bit.  The base is read from its slot once and stays in
      // registers with the accumulator; the exponent's words come from the kernel arguments by scalar loads.  No table.
      case ADMIT >= TAPE_POW ? VDF_TAPE_POW : TAPE_NO_OP: {
        uint32_t q = 8, word = 0;                    // words of the exponent still to read, and the one being read
        while (q && (word = tape.consts[b].v[q - 1]) == 0) --q;
        if (q == 0) { v = fe_one<P>(); break; }      // E = 0
        const Fe<P> y = slot_load<P>(slots, a, lane);
        v = y;                                       // the top set bit
        int bit = 31 - __builtin_clz(word);
        for (;;) {
#pragma unroll 1
          while (bit-- > 0) {
            v = fe_sqr(v);
            if ((word >> bit) & 1) v = fe_mul(v, y);
          }
          if (--q == 0) break;
          word = tape.consts[b].v[q - 1];
          bit = 32;
        }
        break;
      }
      // a power by a caller-supplied addition chain, interpreted as k_forward_walk (minroot.hip) interprets the built-in one.  The
      // accumulator stays in registers; the chain's temporaries are n_tmp more lane-private slots of LDS from tmp0, same
      // [slot][half][lane] layout.  The step words and the trip counts come from tape.consts by scalar loads (the chain is the same
      // for every lane).  ONE squaring site and ONE product site, both in loops: the chain is not inlined.
      //
      // Bound: inside a chain the values are in the lazy domain of fe.cuh.  The base is canonical (every slot is).  A lazy square or
      // product of operands below 2m + k eps is below 2m + (k + 1) eps.  On any path from the base to a value every squaring doubles
      // the exponent and every product raises it, and a valid chain's exponents stay below 2^256: at most 255 squarings; a path
      // passes a step at most once: at most 95 products.  So every value stays below 2m + 350 eps < 2^256 (eps ~ 2^126), the GENERAL
      // lazy forms apply (the _t31 forms carry a nine-product bound that a chain exceeds), and fe_canon's two subtractions make the
      // result canonical.
      case ADMIT >= TAPE_POWC ? VDF_TAPE_POWC : TAPE_NO_OP + 1: {
        const uint32_t* const cw = &tape.consts[0].v[0] + b * 8;      // word 0: n_steps | n_tmp << 8; word 1 + k: step k (the launcher checked all)
        const uint32_t n_steps = cw[0] & 0xFF;
        v = slot_load<P>(slots, a, lane);
        slot_store<P>(slots, tmp0, lane, v);         // T[0] = the base
#pragma unroll 1
        for (uint32_t k = 0; k < n_steps; ++k) {
          const uint32_t st = cw[1 + k];
          const uint32_t src = st & 0xFF, mul = (st >> 16) & 0xFF, keep = st >> 24;
          if (src != VDF_POW_ACC) v = slot_load<P>(slots, tmp0 + src, lane);
#pragma unroll 1
          for (uint32_t q = (st >> 8) & 0xFF; q; --q) v = fe_sqr_lazy(v);
          if (mul != VDF_POW_NONE) v = fe_mul_lazy(v, slot_load<P>(slots, tmp0 + mul, lane));
          if (keep != VDF_POW_NONE) slot_store<P>(slots, tmp0 + keep, lane, v);
        }
        v = fe_canon(v);                             // below 2m + 350 eps (above): two conditional subtractions
        break;
      }
      case HAS_TAB ? VDF_TAPE_TAB : TAPE_NO_OP + 2:
        if constexpr (HAS_TAB) v = tab.template load<P>(a);
        break;
      default:                       // VDF_TAPE_OUT (the launcher admits no other opcode)
        io.store_out(slots, lane, b, slot_load<P>(slots, a, lane));
        continue;
    }
    slot_store<P>(slots, dst, lane, v);
  }
}

template <class P>
__global__ __launch_bounds__(64) void k_round_tape(TapeArgs tape, const char* __restrict__ advice, uint64_t t, char* __restrict__ out) {
  extern __shared__ uint4 tape_slots[];
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint32_t lane = threadIdx.x;
  const uint64_t j = (uint64_t)blockIdx.x * 64 + lane;
  if (j >= t) return;
  const RoundIO<P> io = {advice + j * tape.n_adv * 32, out + j * tape.n_vars * 32, 0};
  tape_round<P, TAPE_BASE>(tape, tape_slots, lane, j, io);
}

// k_round_tape for a tape that holds a TAB: the row of repetition j, taken once per thread
template <class P>
__global__ __launch_bounds__(64) void k_round_tape_tab(TapeArgs tape, const char* __restrict__ advice, uint64_t t, char* __restrict__ out, TabArgs ta) {
  extern __shared__ uint4 tape_slots[];
  __builtin_amdgcn_s_setprio(3);
  const uint32_t lane = threadIdx.x;
  const uint64_t j = (uint64_t)blockIdx.x * 64 + lane;
  if (j >= t) return;
  const RoundIO<P> io = {advice + j * tape.n_adv * 32, out + j * tape.n_vars * 32, 0};
  TabIO tab = tab_io(ta);
  tab.at(j);
  tape_round<P, TAPE_BASE>(tape, tape_slots, lane, j, io, 0, tab);
}

// k_round_tape for `lanes` advice arrays in ONE launch (vdf_hip.h vdf_round_tape_run_lanes): the lane is the grid's second dimension,
// so it is a scalar like the tape: the lane's advice, its variables and its own n_inv invariants -- all lanes' invariants share the
// 512-byte block of the arguments, lane-major -- are reached through scalar offsets.
struct LaneRunArgs { uint64_t t, lane_stride; uint32_t n_inv, pad; };
static_assert(sizeof(TapeArgs) + sizeof(LaneRunArgs) + 16 <= 4096, "the tape travels in the kernel-argument segment");

template <class P>
__global__ __launch_bounds__(64) void k_round_tape_lanes(TapeArgs tape, LaneRunArgs la, const char* __restrict__ advice, char* __restrict__ out) {
  extern __shared__ uint4 tape_slots[];
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint32_t lane = threadIdx.x;
  const uint64_t j = (uint64_t)blockIdx.x * 64 + lane;
  if (j >= la.t) return;
  const uint64_t l = blockIdx.y;                     // (wave-uniform)
  const uint32_t inv0 = (uint32_t)l * la.n_inv;
  const RoundIO<P> io = {advice + (l * la.lane_stride + j) * tape.n_adv * 32, out + (l * la.t + j) * tape.n_vars * 32, inv0};
  tape_round<P, TAPE_BASE>(tape, tape_slots, lane, j, io);
}

template <class P>
__global__ __launch_bounds__(64) void k_round_tape_lanes_tab(TapeArgs tape, LaneRunArgs la, const char* __restrict__ advice, char* __restrict__ out,
                                                             TabArgs ta) {
  extern __shared__ uint4 tape_slots[];
  __builtin_amdgcn_s_setprio(3);
  const uint32_t lane = threadIdx.x;
  const uint64_t j = (uint64_t)blockIdx.x * 64 + lane;
  if (j >= la.t) return;
  const uint64_t l = blockIdx.y;                     // (wave-uniform)
  const uint32_t inv0 = (uint32_t)l * la.n_inv;
  const RoundIO<P> io = {advice + (l * la.lane_stride + j) * tape.n_adv * 32, out + (l * la.t + j) * tape.n_vars * 32, inv0};
  TabIO tab = tab_io(ta);
  tab.at(j);
  tape_round<P, TAPE_BASE>(tape, tape_slots, lane, j, io, 0, tab);
}

// ---- walk tapes: the advice itself, rebuilt from checkpoints (vdf_hip.h vdf_round_tape_walk) ---------------------------------
// k_inverse_walk's launch (one lane per walk, workgroups of one wavefront, wave priority left at 0: background work beside a
// prover) around the interpreter.  Two entries of n_adv slots follow the value file in LDS: the one the walk stands on and the one
// the round produces, swapped on the round's parity -- an OUT to column c never touches what a later ADV of column c reads.  The
// slot numbers of both are scalars; nothing is indexed by a run-time value outside LDS.  A round is sequential after the one before
// it, so unlike k_round_tape the interpreter's scalar loads of the tape recur every round: they stay in the scalar cache (2.5 KiB
// of arguments).
//
// In lanes (vdf_hip.h vdf_round_tape_walk_lanes) the groups are numbered step-major, lane-minor: group G = g * lanes + l is lane l
// of step g.  There the lane is a per-thread value -- one wavefront holds walks of several lanes -- and the kernel arguments
// indexed by it would go to scratch.  So each thread selects its own j_base and invariants ONCE, before the rounds, in a uniform
// loop over the at most VDF_TAPE_MAX_LANES argument elements (scalar loads, a select per element), and keeps the invariants in n_inv
// more lane-private slots of LDS behind the two entries: an INV op is then a slot load like any other.
struct WalkArgs {
  uint64_t n, walk_stride, top, group, group_stride, j_base, j_group_step;
  uint32_t rounds, n_slots, heads, pad;
};
struct WalkLanesArgs {
  WalkArgs w;
  uint32_t lanes, n_inv;
  uint64_t j_base[VDF_TAPE_MAX_LANES];
};
static_assert(sizeof(TapeArgs) + sizeof(WalkLanesArgs) + 32 <= 4096, "the tape travels in the kernel-argument segment");

// wl: the lanes form's arguments behind wa (= wl->w), null for k_tape_walk
template <class P, bool LANES, class TAB = NoTab>
__device__ __forceinline__ void tape_walk(const TapeArgs& tape, const WalkArgs& wa, const WalkLanesArgs* wl, uint4* slots, char* entries,
                                          char* trace, const char* expect, int32_t* ok, TAB tab = TAB()) {
  constexpr bool HAS_TAB = !std::is_same<TAB, NoTab>::value;
  const uint32_t lane = threadIdx.x;
  const uint64_t w = (uint64_t)blockIdx.x * 64 + lane;
  if (w >= wa.n) return;                             // (no barrier below: a lane touches only its own words of LDS)
  const uint32_t na = tape.n_adv;
  const size_t esz = (size_t)na * 32;
  char* const ep = entries + w * esz;
  const uint64_t G = w / wa.group, first = (w % wa.group) * wa.walk_stride + wa.top;      // local index of the entry the walk stands on
  uint64_t g = G, jb = wa.j_base;
  uint32_t stand = wa.n_slots, prod = wa.n_slots + na;
  const uint32_t inv0 = wa.n_slots + 2 * na;
  if constexpr (LANES) {
    g = G / wl->lanes;
    const uint32_t l = (uint32_t)(G % wl->lanes);
    jb = 0;
#pragma unroll 1
    for (uint32_t q = 0; q < wl->lanes; ++q) {
      const uint64_t x = wl->j_base[q];
      jb = q == l ? x : jb;
    }
#pragma unroll 1
    for (uint32_t k = 0; k < wl->n_inv; ++k) {
      Fe<P> v = fe_zero<P>();
#pragma unroll 1
      for (uint32_t q = 0; q < wl->lanes; ++q) {
        const Fe<P> x = tape_fe<P>(tape.inv[q * wl->n_inv + k]);
#pragma unroll
        for (int i = 0; i < 8; ++i) v.v[i] = q == l ? x.v[i] : v.v[i];
      }
      slot_store<P>(slots, inv0 + k, lane, v);
    }
  }
  for (uint32_t c = 0; c < na; ++c) slot_store<P>(slots, stand + c, lane, fe_load<P>(ep + c * 32));
  char* tp = trace ? trace + (G * wa.group_stride + first) * esz : nullptr;
  uint64_t j = jb + g * wa.j_group_step + first - 1;
  if constexpr (HAS_TAB) tab.at(j);
#pragma unroll 1
  for (uint32_t r = 0; r < wa.rounds; ++r, --j) {
    if (tp) {
      for (uint32_t c = 0; c < na; ++c) fe_store<P>(tp + c * 32, slot_load<P>(slots, stand + c, lane));
      tp -= esz;
    }
    const WalkIO<P, LANES> io = {stand, prod, inv0};
    tape_round<P, TAPE_BASE>(tape, slots, lane, j, io, 0, tab);
    const uint32_t t = stand; stand = prod; prod = t;
    if constexpr (HAS_TAB) tab.down(j - 1);
  }
  // where the walk landed: back into entries, to the head of its group's trace, and against the checkpoint
  uint32_t diff = 0;
  const bool head = tp && wa.heads && w % wa.group == 0;
  for (uint32_t c = 0; c < na; ++c) {
    const Fe<P> v = slot_load<P>(slots, stand + c, lane);
    fe_store<P>(ep + c * 32, v);
    if (head) fe_store<P>(tp + c * 32, v);
    if (expect) {
      const Fe<P> e = fe_load<P>(expect + w * esz + c * 32);
#pragma unroll
      for (int q = 0; q < 8; ++q) diff |= v.v[q] ^ e.v[q];
    }
  }
  if (expect) ok[w] = diff == 0;
}

template <class P>
__global__ __launch_bounds__(64) void k_tape_walk(TapeArgs tape, WalkArgs wa, char* __restrict__ entries, char* __restrict__ trace,
                                                  const char* __restrict__ expect, int32_t* __restrict__ ok) {
  extern __shared__ uint4 tape_slots[];
  tape_walk<P, false>(tape, wa, nullptr, tape_slots, entries, trace, expect, ok);
}

template <class P>
__global__ __launch_bounds__(64) void k_tape_walk_lanes(TapeArgs tape, WalkLanesArgs wl, char* __restrict__ entries, char* __restrict__ trace,
                                                        const char* __restrict__ expect, int32_t* __restrict__ ok) {
  extern __shared__ uint4 tape_slots[];
  tape_walk<P, true>(tape, wl.w, &wl, tape_slots, entries, trace, expect, ok);
}

template <class P>
__global__ __launch_bounds__(64) void k_tape_walk_tab(TapeArgs tape, WalkArgs wa, char* __restrict__ entries, char* __restrict__ trace,
                                                      const char* __restrict__ expect, int32_t* __restrict__ ok, TabArgs ta) {
  extern __shared__ uint4 tape_slots[];
  tape_walk<P, false>(tape, wa, nullptr, tape_slots, entries, trace, expect, ok, tab_io(ta));
}

template <class P>
__global__ __launch_bounds__(64) void k_tape_walk_lanes_tab(TapeArgs tape, WalkLanesArgs wl, char* __restrict__ entries, char* __restrict__ trace,
                                                            const char* __restrict__ expect, int32_t* __restrict__ ok, TabArgs ta) {
  extern __shared__ uint4 tape_slots[];
  tape_walk<P, true>(tape, wl.w, &wl, tape_slots, entries, trace, expect, ok, tab_io(ta));
}

// ---- forward walk tapes: the chain itself, many at once (vdf_hip.h vdf_round_tape_forward_walk) -------------------------------
// k_tape_walk ascending: the same launch (one lane per walk, workgroups of one wavefront, wave priority left at 0), the same
// interpreter and the same two entries behind the value file in LDS, swapped each round; what a round produces goes to the trace
// and, every `every` rounds, to the checkpoints, in k_forward_walk's layout.  k_tape_forward_walk admits VDF_TAPE_POW on top of the
// base ops; k_tape_forward_walk_chain, for a tape that holds a VDF_TAPE_POWC, admits that too and keeps the chains' temporaries in
// n_tmp more slots behind the two entries -- every other tape runs the kernel that does not carry the chain interpreter.
struct ForwardArgs {
  uint64_t n, walk_stride, cp_stride, every, base, j_base, j_walk_step;
  uint32_t rounds, n_slots;
};
static_assert(sizeof(TapeArgs) + sizeof(ForwardArgs) + 24 <= 4096, "the tape travels in the kernel-argument segment");

template <class P, int ADMIT, class TAB = NoTab>
__device__ __forceinline__ void tape_forward_walk(const TapeArgs& tape, const ForwardArgs& fa, uint4* slots, char* entries, char* checkpoints,
                                                  char* trace, TAB tab = TAB()) {
  constexpr bool HAS_TAB = !std::is_same<TAB, NoTab>::value;
  const uint32_t lane = threadIdx.x;
  const uint64_t w = (uint64_t)blockIdx.x * 64 + lane;
  if (w >= fa.n) return;                             // (no barrier below: a lane touches only its own words of LDS)
  const uint32_t na = tape.n_adv;
  const size_t esz = (size_t)na * 32;
  char* const ep = entries + w * esz;
  uint32_t stand = fa.n_slots, prod = fa.n_slots + na;
  const uint32_t tmp0 = fa.n_slots + 2 * na;         // T[0] of a chain
  for (uint32_t c = 0; c < na; ++c) slot_store<P>(slots, stand + c, lane, fe_load<P>(ep + c * 32));
  // entry base + r + 1 after round r; checkpoint (base + r + 1) / every when `every` divides base + r + 1
  char* tp = trace ? trace + (w * fa.walk_stride + fa.base + 1) * esz : nullptr;
  uint64_t cp_left = checkpoints ? fa.every - fa.base % fa.every : 0;
  char* cp = checkpoints ? checkpoints + (w * fa.cp_stride + fa.base / fa.every + 1) * esz : nullptr;
  uint64_t j = fa.j_base + w * fa.j_walk_step + fa.base;
  if constexpr (HAS_TAB) tab.at(j);
#pragma unroll 1
  for (uint32_t r = 0; r < fa.rounds; ++r, ++j) {
    const WalkIO<P, false> io = {stand, prod, 0};
    tape_round<P, ADMIT>(tape, slots, lane, j, io, tmp0, tab);
    if constexpr (HAS_TAB) tab.up(j + 1);
    const uint32_t t = stand; stand = prod; prod = t;
    if (tp) {
      for (uint32_t c = 0; c < na; ++c) fe_store<P>(tp + c * 32, slot_load<P>(slots, stand + c, lane));
      tp += esz;
    }
    if (cp && --cp_left == 0) {
      for (uint32_t c = 0; c < na; ++c) fe_store<P>(cp + c * 32, slot_load<P>(slots, stand + c, lane));
      cp += esz;
      cp_left = fa.every;
    }
  }
  for (uint32_t c = 0; c < na; ++c) fe_store<P>(ep + c * 32, slot_load<P>(slots, stand + c, lane));
}

template <class P>
__global__ __launch_bounds__(64) void k_tape_forward_walk(TapeArgs tape, ForwardArgs fa, char* __restrict__ entries,
                                                          char* __restrict__ checkpoints, char* __restrict__ trace) {
  extern __shared__ uint4 tape_slots[];
  tape_forward_walk<P, TAPE_POW>(tape, fa, tape_slots, entries, checkpoints, trace);
}

template <class P>
__global__ __launch_bounds__(64) void k_tape_forward_walk_chain(TapeArgs tape, ForwardArgs fa, char* __restrict__ entries,
                                                                char* __restrict__ checkpoints, char* __restrict__ trace) {
  extern __shared__ uint4 tape_slots[];
  tape_forward_walk<P, TAPE_POWC>(tape, fa, tape_slots, entries, checkpoints, trace);
}
// a forward tape that holds a TAB: ONE kernel that admits POW, POWC and TAB together
template <class P>
__global__ __launch_bounds__(64) void k_tape_forward_walk_tab(TapeArgs tape, ForwardArgs fa, char* __restrict__ entries,
                                                              char* __restrict__ checkpoints, char* __restrict__ trace, TabArgs ta) {
  extern __shared__ uint4 tape_slots[];
  tape_forward_walk<P, TAPE_POWC>(tape, fa, tape_slots, entries, checkpoints, trace, tab_io(ta));
}

// ---- traces rebuilt by forward tapes: k_tape_walk_lanes ascending (vdf_hip.h vdf_round_tape_rebuild_lanes) ---------------------
// One lane per checkpoint interval, for a round with no cheap inverse: the walk stands on the checkpoint BELOW its interval, runs the
// chain's own forward tape (POW, POWC and in the _tab kernel TAB admitted), writes every entry it produces where vdf_cs_repeat reads
// its advice, and is compared with the checkpoint ABOVE.  The launch, the interpreter and the two entries swapped each round are
// k_tape_forward_walk_chain's; the groups, the per-lane counter and the invariants kept in n_inv slots of LDS are
// k_tape_walk_lanes'.  Which walk stands where and sees which counter is tape_launch.h's, shared with the host restatement.
// LDS: the value file, the two entries, the chains' temporaries, the lane's invariants.
struct RebuildArgs {
  uint64_t n, walk_stride, base, group, group_stride, j_group_step;
  uint32_t rounds, n_slots, heads, lanes, n_inv, chain_tmp;
  uint64_t j_base[VDF_TAPE_MAX_LANES];
};
static_assert(sizeof(TapeArgs) + sizeof(RebuildArgs) + 32 + sizeof(TabArgs) <= 4096, "the tape travels in the kernel-argument segment");

template <class P, class TAB = NoTab>
__device__ __forceinline__ void tape_rebuild(const TapeArgs& tape, const RebuildArgs& ra, uint4* slots, char* entries, char* trace,
                                             const char* expect, int32_t* ok, TAB tab = TAB()) {
  constexpr bool HAS_TAB = !std::is_same<TAB, NoTab>::value;
  const uint32_t lane = threadIdx.x;
  const uint64_t w = (uint64_t)blockIdx.x * 64 + lane;
  if (w >= ra.n) return;                             // (no barrier below: a lane touches only its own words of LDS)
  const uint32_t na = tape.n_adv;
  const size_t esz = (size_t)na * 32;
  char* const ep = entries + w * esz;
  const vdflaunch::Place p = vdflaunch::place(w, ra.group, ra.walk_stride, ra.base, ra.lanes);
  uint32_t stand = ra.n_slots, prod = ra.n_slots + na;
  const uint32_t tmp0 = ra.n_slots + 2 * na, inv0 = tmp0 + ra.chain_tmp;
  // the lane is a per-thread value: its counter and invariants are selected ONCE, in uniform loops over the argument elements
  uint64_t jb = 0;
#pragma unroll 1
  for (uint32_t q = 0; q < ra.lanes; ++q) {
    const uint64_t x = ra.j_base[q];
    jb = q == p.l ? x : jb;
  }
#pragma unroll 1
  for (uint32_t k = 0; k < ra.n_inv; ++k) {
    Fe<P> v = fe_zero<P>();
#pragma unroll 1
    for (uint32_t q = 0; q < ra.lanes; ++q) {
      const Fe<P> x = tape_fe<P>(tape.inv[q * ra.n_inv + k]);
#pragma unroll
      for (int i = 0; i < 8; ++i) v.v[i] = q == p.l ? x.v[i] : v.v[i];
    }
    slot_store<P>(slots, inv0 + k, lane, v);
  }
  char* tp = trace ? trace + vdflaunch::trace_entry(p, ra.group_stride, p.k) * esz : nullptr;      // the entry stood on
  const bool head = tp && ra.heads && p.first;
  for (uint32_t c = 0; c < na; ++c) {
    const Fe<P> v = fe_load<P>(ep + c * 32);
    slot_store<P>(slots, stand + c, lane, v);
    if (head) fe_store<P>(tp + c * 32, v);
  }
  uint64_t j = vdflaunch::counter(p, jb, ra.j_group_step);
  if constexpr (HAS_TAB) tab.at(j);
#pragma unroll 1
  for (uint32_t r = 0; r < ra.rounds; ++r, ++j) {
    const WalkIO<P, true> io = {stand, prod, inv0};
    tape_round<P, TAPE_POWC>(tape, slots, lane, j, io, tmp0, tab);
    if constexpr (HAS_TAB) tab.up(j + 1);
    const uint32_t t = stand; stand = prod; prod = t;
    if (tp) {
      tp += esz;
      for (uint32_t c = 0; c < na; ++c) fe_store<P>(tp + c * 32, slot_load<P>(slots, stand + c, lane));
    }
  }
  // where the walk stands now: back into entries, and against the checkpoint above
  uint32_t diff = 0;
  for (uint32_t c = 0; c < na; ++c) {
    const Fe<P> v = slot_load<P>(slots, stand + c, lane);
    fe_store<P>(ep + c * 32, v);
    if (expect) {
      const Fe<P> e = fe_load<P>(expect + w * esz + c * 32);
#pragma unroll
      for (int q = 0; q < 8; ++q) diff |= v.v[q] ^ e.v[q];
    }
  }
  if (expect) ok[w] = diff == 0;
}

template <class P>
__global__ __launch_bounds__(64) void k_tape_rebuild_lanes(TapeArgs tape, RebuildArgs ra, char* __restrict__ entries, char* __restrict__ trace,
                                                           const char* __restrict__ expect, int32_t* __restrict__ ok) {
  extern __shared__ uint4 tape_slots[];
  tape_rebuild<P>(tape, ra, tape_slots, entries, trace, expect, ok);
}

template <class P>
__global__ __launch_bounds__(64) void k_tape_rebuild_lanes_tab(TapeArgs tape, RebuildArgs ra, char* __restrict__ entries,
                                                               char* __restrict__ trace, const char* __restrict__ expect,
                                                               int32_t* __restrict__ ok, TabArgs ta) {
  extern __shared__ uint4 tape_slots[];
  tape_rebuild<P>(tape, ra, tape_slots, entries, trace, expect, ok, tab_io(ta));
}
// ---- periodic rows: the cross term of the rows of such rounds without the sparse matrices (vdf_hip.h vdf_periodic_rows) --------
// k_nifs_cross_minroot_forward_lanes for a round the library did not write: one row per lane, workgroups of 256, every running /
// fresh vector read and written as contiguous 32-byte elements.  What the hand-written stencil has in its code -- which columns a
// row reads, with which coefficients -- is a table here: it travels in the kernel arguments, is staged ONCE per workgroup into LDS
// (2 KiB), and every lane fetches the terms of its own row (i mod n_cons) from there.  The loop over term slots is uniform (up to the
// longest list of each matrix, a lane without a term in a slot gathers column 0 and drops it): the gathers of a slot, one per matrix,
// are all in flight before the first is used, and a1, b1, c1 before any of them.  A product is taken only in the lanes whose
// coefficient is neither 1 nor -1 (the launcher classifies them); an affine coefficient c0 + (j - j0) c1 skips its second product
// where the gathered value is 1 (the constant's column in a fresh instance).  Nothing private is indexed by a run-time value.
// (One repetition per thread with the description read by scalar loads would have uniform control, but strides every stream by
// n_cons * 32 bytes: a wavefront's store would touch 64 separate cache lines per vector.)
enum { PT_ONE = 0, PT_MINUS_ONE = 1, PT_MUL = 2, PT_AFFINE_UNIT = 3, PT_AFFINE = 4 };      // how a term's coefficient is applied
struct PeriodicArgs {
  uint32_t n_cons, n_vars, n_terms, n_consts;
  uint32_t max_len[3], rows;                        // the longest list per matrix; rows = reps * n_cons
  uint64_t j_first, j0;
  uint64_t seg_begin, row0;
  uint16_t row_start[3 * VDF_PERIODIC_MAX_ROWS + 4];
  uint32_t terms[2 * VDF_PERIODIC_MAX_TERMS];       // col, then kind | how << 8 | c0 << 16 | c1 << 24
  TapeFe consts[VDF_PERIODIC_MAX_CONSTS];
};
static_assert(VDF_PERIODIC_MAX_STARTS == 3 * VDF_PERIODIC_MAX_ROWS + 1, "row_start: one entry per row and matrix, and the end");
static_assert(sizeof(PeriodicArgs) + 8 * 8 + sizeof(TapeFe) <= 4096, "the description travels in the kernel-argument segment");

template <class P> __device__ __forceinline__ Fe<P> lds_fe(const uint4* t, uint32_t k) {
  const uint4 lo = t[2 * k], hi = t[2 * k + 1];
  Fe<P> r;
  r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
  r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
  return r;
}

template <class P>
__global__ __launch_bounds__(256) void k_nifs_cross_periodic(PeriodicArgs pa, const char* __restrict__ z2, const char* __restrict__ az1,
                                                             const char* __restrict__ bz1, const char* __restrict__ cz1, TapeFe u1,
                                                             char* __restrict__ az2, char* __restrict__ bz2, char* __restrict__ cz2,
                                                             char* __restrict__ T) {
  __shared__ uint32_t s_terms[2 * VDF_PERIODIC_MAX_TERMS];
  __shared__ uint32_t s_start[3 * VDF_PERIODIC_MAX_ROWS + 1];
  __shared__ uint4 s_consts[2 * VDF_PERIODIC_MAX_CONSTS];
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  for (uint32_t w = threadIdx.x; w < 2 * pa.n_terms; w += 256) s_terms[w] = pa.terms[w];
  for (uint32_t w = threadIdx.x; w <= 3 * pa.n_cons; w += 256) s_start[w] = pa.row_start[w];
  for (uint32_t w = threadIdx.x; w < 8 * pa.n_consts; w += 256) reinterpret_cast<uint32_t*>(s_consts)[w] = pa.consts[w >> 3].v[w & 7];
  __syncthreads();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= pa.rows) return;
  const uint32_t rep = i / pa.n_cons, c = i - rep * pa.n_cons;
  const uint64_t j = pa.j_first + rep;
  const size_t r = pa.row0 + i;
  const Fe<P> a1 = fe_load<P>(az1 + r * 32), b1 = fe_load<P>(bz1 + r * 32), c1 = fe_load<P>(cz1 + r * 32);
  const size_t seg = pa.seg_begin + j * pa.n_vars;                   // column of this repetition's first variable
  const uint32_t st0 = s_start[3 * c], st1 = s_start[3 * c + 1], st2 = s_start[3 * c + 2], st3 = s_start[3 * c + 3];
  const uint32_t lo[3] = {st0, st1, st2}, hi[3] = {st1, st2, st3};
  Fe<P> acc[3] = {fe_zero<P>(), fe_zero<P>(), fe_zero<P>()};
  const uint32_t longest = max(pa.max_len[0], max(pa.max_len[1], pa.max_len[2]));
#pragma unroll 1
  for (uint32_t s = 0; s < longest; ++s) {
    bool has[3];
    uint32_t how[3];
    Fe<P> v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      has[k] = false; how[k] = 0;
      if (s >= pa.max_len[k]) continue;                              // (uniform)
      has[k] = lo[k] + s < hi[k];
      const uint32_t e = has[k] ? lo[k] + s : 0u;
      const uint32_t col = s_terms[2 * e];
      how[k] = s_terms[2 * e + 1];
      const size_t at = (how[k] & 0xFF) == VDF_TERM_SEG ? seg + (size_t)(int64_t)(int32_t)col : (size_t)col;
      v[k] = fe_load<P>(z2 + (has[k] ? at : (size_t)0) * 32);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (!has[k]) continue;
      const uint32_t mode = (how[k] >> 8) & 0xFF, k0 = (how[k] >> 16) & 0xFF, k1 = how[k] >> 24;
      if (mode == PT_ONE) acc[k] = fe_add(acc[k], v[k]);
      else if (mode == PT_MINUS_ONE) acc[k] = fe_sub(acc[k], v[k]);
      else {
        Fe<P> coef = lds_fe<P>(s_consts, k0);
        if (mode != PT_MUL) {
          const uint64_t d = j - pa.j0;
          Fe<P> m = fe_from_count<P>(d);
          if (mode == PT_AFFINE) m = fe_mul(m, lds_fe<P>(s_consts, k1));
          coef = fe_add(coef, m);
        }
        acc[k] = fe_add(acc[k], mode != PT_MUL && fe_eq(v[k], fe_one<P>()) ? coef : fe_mul(coef, v[k]));
      }
    }
  }
  cross_finish<P>(az2, bz2, cz2, T, r, a1, b1, c1, tape_fe<P>(u1), acc[0], acc[1], acc[2]);
}

using namespace vdflaunch;      // the launch kinds and the verdicts (tape_launch.h)
static TapeFe tape_val(const vdf_fe* p) { TapeFe v; std::memcpy(&v, p, 32); return v; }
static Status status_of(const Verdict& v) { return Status{v.code, v.why}; }
// Every refusal of a launch is tape_launch.h's (with tape_rules.h's behind it), made before anything here runs: what is left is the
// words of TapeArgs.  inv holds lanes * n_inv elements, lane-major; all of them go into the block of VDF_TAPE_MAX_INV.
static TapeArgs pack_tape(const vdf_round_tape* tp, const vdf_fe* inv, size_t lanes = 1) {
  TapeArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_ops = (uint32_t)tp->n_ops; a.n_vars = tp->n_vars; a.n_adv = tp->n_adv;
  for (size_t i = 0; i < tp->n_ops; ++i) {
    const vdf_tape_op& o = tp->ops[i];
    a.ops[i] = (uint32_t)o.op | (uint32_t)o.dst << 8 | (uint32_t)o.a << 16 | (uint32_t)o.b << 24;
  }
  for (size_t k = 0; k < tp->n_consts; ++k) a.consts[k] = tape_val(&tp->consts[k]);
  for (size_t k = 0; k < lanes * tp->n_inv; ++k) a.inv[k] = tape_val(&inv[k]);
  return a;
}

// the table of a tape that holds a TAB, as the k_*_tab kernels take it (the abi has checked that a kernel may read it in place)
static TabArgs tab_args(const vdf_round_tape* tp) { return TabArgs{cbytes_of(tp->table), tp->tab_rows, tp->tab_cols}; }

Status vec_round_tape(int field, const vdf_round_tape* tp, uint64_t t, const vdf_fe* inv, const void* advice, void* out, hipStream_t s) {
  const Verdict v = round_launch(RUN, tp, t, 1, inv, 0);
  VDF_TRY(status_of(v));
  const TapeArgs a = pack_tape(tp, inv);
  // advice read + variables written per repetition
  KTimer kt(s, v.ti.tab ? "k_round_tape_tab" : "k_round_tape", 32.0 * (tp->n_adv + tp->n_vars) * t);
  const dim3 grid((unsigned)((t + 63) / 64));
  const size_t lds = lds_bytes(RUN, tp, v.ti);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    if (v.ti.tab) hipLaunchKernelGGL((k_round_tape_tab<P>), grid, dim3(64), lds, s, a, cbytes_of(advice), t, bytes_of(out), tab_args(tp));
    else hipLaunchKernelGGL((k_round_tape<P>), grid, dim3(64), lds, s, a, cbytes_of(advice), t, bytes_of(out));
  });
}

static WalkArgs walk_args(const vdf_round_tape* tp, size_t n, uint64_t rounds, size_t walk_stride, size_t top, uint64_t group, uint64_t group_stride,
                          uint64_t j_base, uint64_t j_group_step, int heads) {
  groups(n, &group, &group_stride);
  WalkArgs wa;
  std::memset(&wa, 0, sizeof(wa));
  wa.n = n; wa.walk_stride = walk_stride; wa.top = top; wa.group = group; wa.group_stride = group_stride;
  wa.j_base = j_base; wa.j_group_step = j_group_step;
  wa.rounds = (uint32_t)rounds; wa.n_slots = tp->n_slots; wa.heads = heads != 0;
  return wa;
}

Status vec_round_tape_walk(int field, const vdf_round_tape* tp, const vdf_fe* inv, void* entries, size_t n, uint64_t rounds, void* trace,
                           size_t walk_stride, size_t top, size_t group, size_t group_stride, uint64_t j_base, uint64_t j_group_step,
                           int heads, const void* expect, int32_t* ok, hipStream_t s) {
  VDF_TRY(check_field(field));
  const Verdict v = walk_launch({WALK, tp, 1, inv, nullptr, n, rounds, entries, trace, walk_stride, top, group, heads, expect, ok, nullptr, 0});
  if (v.refused() || v.nothing) return status_of(v);
  const TapeArgs a = pack_tape(tp, inv);
  const WalkArgs wa = walk_args(tp, n, rounds, walk_stride, top, group, group_stride, j_base, j_group_step, heads);
  KTimer kt(s, v.ti.tab ? "k_tape_walk_tab" : "k_tape_walk", trace ? 32.0 * tp->n_adv * (double)n * (double)rounds : 0.0);
  const size_t lds = lds_bytes(WALK, tp, v.ti);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    if (v.ti.tab)
      hipLaunchKernelGGL((k_tape_walk_tab<P>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, wa, bytes_of(entries), bytes_of(trace),
                         cbytes_of(expect), ok, tab_args(tp));
    else
      hipLaunchKernelGGL((k_tape_walk<P>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, wa, bytes_of(entries), bytes_of(trace),
                         cbytes_of(expect), ok);
  });
}

Status vec_round_tape_lanes(int field, const vdf_round_tape* tp, uint64_t t, size_t lanes, const vdf_fe* inv, const void* advice,
                            size_t lane_stride, void* out, hipStream_t s) {
  VDF_TRY(check_field(field));
  const Verdict v = round_launch(RUN_LANES, tp, t, lanes, inv, lane_stride);
  VDF_TRY(status_of(v));
  const TapeArgs a = pack_tape(tp, inv, lanes);
  LaneRunArgs la;
  std::memset(&la, 0, sizeof(la));
  la.t = t; la.lane_stride = lane_stride; la.n_inv = tp->n_inv;
  KTimer kt(s, v.ti.tab ? "k_round_tape_lanes_tab" : "k_round_tape_lanes", 32.0 * (tp->n_adv + tp->n_vars) * t * lanes);
  const dim3 grid((unsigned)((t + 63) / 64), (unsigned)lanes);
  const size_t lds = lds_bytes(RUN_LANES, tp, v.ti);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    if (v.ti.tab) hipLaunchKernelGGL((k_round_tape_lanes_tab<P>), grid, dim3(64), lds, s, a, la, cbytes_of(advice), bytes_of(out), tab_args(tp));
    else hipLaunchKernelGGL((k_round_tape_lanes<P>), grid, dim3(64), lds, s, a, la, cbytes_of(advice), bytes_of(out));
  });
}

Status vec_round_tape_walk_lanes(int field, const vdf_round_tape* tp, size_t lanes, const vdf_fe* inv, void* entries, size_t n, uint64_t rounds,
                                 void* trace, size_t walk_stride, size_t top, size_t group, size_t group_stride, const uint64_t* j_base,
                                 uint64_t j_group_step, int heads, const void* expect, int32_t* ok, hipStream_t s) {
  VDF_TRY(check_field(field));
  const Verdict v = walk_launch({WALK_LANES, tp, lanes, inv, j_base, n, rounds, entries, trace, walk_stride, top, group, heads, expect, ok, nullptr, 0});
  if (v.refused() || v.nothing) return status_of(v);
  const TapeArgs a = pack_tape(tp, inv, lanes);
  WalkLanesArgs wl;
  std::memset(&wl, 0, sizeof(wl));
  wl.w = walk_args(tp, n, rounds, walk_stride, top, group, group_stride, 0, j_group_step, heads);
  wl.lanes = (uint32_t)lanes; wl.n_inv = tp->n_inv;
  for (size_t l = 0; l < lanes; ++l) wl.j_base[l] = j_base[l];
  KTimer kt(s, v.ti.tab ? "k_tape_walk_lanes_tab" : "k_tape_walk_lanes", trace ? 32.0 * tp->n_adv * (double)n * (double)rounds : 0.0);
  const size_t lds = lds_bytes(WALK_LANES, tp, v.ti);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    if (v.ti.tab)
      hipLaunchKernelGGL((k_tape_walk_lanes_tab<P>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, wl, bytes_of(entries), bytes_of(trace),
                         cbytes_of(expect), ok, tab_args(tp));
    else
      hipLaunchKernelGGL((k_tape_walk_lanes<P>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, wl, bytes_of(entries), bytes_of(trace),
                         cbytes_of(expect), ok);
  });
}

// what a forward launch of no rounds is refused for -- the tape's rules, inv, the slot cap -- nothing launched: the rounds one call
// may run, and the rounds vdf_round_tape_eval_batch gives a launch when its caller names no number
Status round_tape_forward_max_rounds(const vdf_round_tape* tp, const vdf_fe* inv, uint64_t* max_rounds, uint64_t* launch_bound) {
  const Verdict v = walk_launch({FORWARD, tp, 1, inv, nullptr, 0, 0, nullptr, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0});
  VDF_TRY(status_of(v));
  *max_rounds = VDF_FORWARD_TAPE_MAX_WORK / v.ti.products;
  *launch_bound = forward_launch_bound(v.ti);
  return Status{};
}

Status vec_round_tape_forward_walk(int field, const vdf_round_tape* tp, const vdf_fe* inv, void* entries, size_t n, uint64_t rounds,
                                   void* checkpoints, uint64_t every, size_t cp_stride, void* trace, size_t walk_stride, uint64_t base,
                                   uint64_t j_base, uint64_t j_walk_step, hipStream_t s) {
  VDF_TRY(check_field(field));
  const Verdict v = walk_launch({FORWARD, tp, 1, inv, nullptr, n, rounds, entries, trace, walk_stride, base, 0, 0, nullptr, nullptr, checkpoints, every});
  if (v.refused() || v.nothing) return status_of(v);
  const TapeArgs a = pack_tape(tp, inv);
  ForwardArgs fa;
  std::memset(&fa, 0, sizeof(fa));
  fa.n = n; fa.walk_stride = walk_stride; fa.cp_stride = cp_stride; fa.every = every; fa.base = base;
  fa.j_base = j_base; fa.j_walk_step = j_walk_step;
  fa.rounds = (uint32_t)rounds; fa.n_slots = tp->n_slots;
  const bool chain = v.ti.chain_tmp != 0;      // a tape with a POWC: the kernel that also runs addition chains; every other tape: the one without
  KTimer kt(s, v.ti.tab ? "k_tape_forward_walk_tab" : chain ? "k_tape_forward_walk_chain" : "k_tape_forward_walk",
            (trace ? 32.0 * tp->n_adv * (double)n * (double)rounds : 0.0) + 64.0 * tp->n_adv * (double)n);
  const size_t lds = lds_bytes(FORWARD, tp, v.ti);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    if (v.ti.tab)                              // a tape with a TAB: the one kernel that admits POW, POWC and TAB (v.ti.chain_tmp may be 0)
      hipLaunchKernelGGL((k_tape_forward_walk_tab<P>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, fa, bytes_of(entries),
                         bytes_of(checkpoints), bytes_of(trace), tab_args(tp));
    else
      hipLaunchKernelGGL(chain ? k_tape_forward_walk_chain<P> : k_tape_forward_walk<P>, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, fa,
                         bytes_of(entries), bytes_of(checkpoints), bytes_of(trace));
  });
}

Status vec_round_tape_rebuild_lanes(int field, const vdf_round_tape* tp, size_t lanes, const vdf_fe* inv, void* entries, size_t n, uint64_t rounds,
                                    void* trace, size_t walk_stride, uint64_t base, size_t group, size_t group_stride, const uint64_t* j_base,
                                    uint64_t j_group_step, int heads, const void* expect, int32_t* ok, hipStream_t s) {
  VDF_TRY(check_field(field));
  const Verdict v = walk_launch({REBUILD, tp, lanes, inv, j_base, n, rounds, entries, trace, walk_stride, base, group, heads, expect, ok, nullptr, 0});
  if (v.refused() || v.nothing) return status_of(v);
  const TapeArgs a = pack_tape(tp, inv, lanes);
  RebuildArgs ra;
  std::memset(&ra, 0, sizeof(ra));
  uint64_t grp = group, gstride = group_stride;
  groups(n, &grp, &gstride);
  ra.n = n; ra.walk_stride = walk_stride; ra.base = base; ra.group = grp; ra.group_stride = gstride; ra.j_group_step = j_group_step;
  ra.rounds = (uint32_t)rounds; ra.n_slots = tp->n_slots; ra.heads = heads != 0; ra.lanes = (uint32_t)lanes; ra.n_inv = tp->n_inv;
  ra.chain_tmp = v.ti.chain_tmp;
  for (size_t l = 0; l < lanes; ++l) ra.j_base[l] = j_base[l];
  KTimer kt(s, v.ti.tab ? "k_tape_rebuild_lanes_tab" : "k_tape_rebuild_lanes", (trace ? 32.0 * tp->n_adv * (double)n * (double)rounds : 0.0) + 64.0 * tp->n_adv * (double)n);
  const size_t lds = lds_bytes(REBUILD, tp, v.ti);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    if (v.ti.tab)
      hipLaunchKernelGGL((k_tape_rebuild_lanes_tab<P>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, ra, bytes_of(entries), bytes_of(trace),
                         cbytes_of(expect), ok, tab_args(tp));
    else
      hipLaunchKernelGGL((k_tape_rebuild_lanes<P>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, ra, bytes_of(entries), bytes_of(trace),
                         cbytes_of(expect), ok);
  });
}

// Everything the description could index out of range is refused by periodic_rules.h, before a launch (vdf_hip.h
// vdf_nifs_cross_term_periodic); here it is packed: the longest list of each matrix, and how each term's coefficient is applied
Status vec_nifs_cross_periodic(int field, const vdf_periodic_rows* pr, uint64_t j_first, uint64_t reps, size_t seg_begin, size_t row0,
                               size_t num_cols, size_t num_cons, const CrossOperands& o, hipStream_t s) {
  VDF_TRY(check_field(field));
  bool nothing = false;
  const std::string why = vdfperiodic::refuse(pr, j_first, reps, seg_begin, row0, num_cols, num_cons, &nothing);
  if (!why.empty()) return Status{VDF_ERR_BAD_ARG, why};
  if (nothing) return Status{};
  PeriodicArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_cons = pr->n_cons; a.n_vars = pr->n_vars; a.n_terms = (uint32_t)pr->n_terms; a.n_consts = (uint32_t)pr->n_consts;
  a.j_first = j_first; a.j0 = pr->j0; a.seg_begin = seg_begin; a.row0 = row0;
  for (uint32_t q = 0; q < 3 * pr->n_cons; ++q) {
    const uint32_t len = pr->row_start[q + 1] - pr->row_start[q];
    if (len > a.max_len[q % 3]) a.max_len[q % 3] = len;
    a.row_start[q + 1] = pr->row_start[q + 1];
  }
  const uint64_t rows = reps * pr->n_cons;
  (void)with_field(field, [&](auto f) -> Status {
    using P = tag_t<decltype(f)>;
    auto fe_of = [&](uint32_t k) { Fe<P> v; std::memcpy(v.v, &pr->consts[k], 32); return v; };
    const Fe<P> p1 = fe_one<P>(), m1 = fe_neg(p1);
    for (size_t e = 0; e < pr->n_terms; ++e) {
      const vdf_periodic_term& t = pr->terms[e];
      uint32_t how = PT_MUL;
      if (t.c1 != VDF_TERM_NO_SLOPE) how = fe_eq(fe_of(t.c1), p1) ? PT_AFFINE_UNIT : PT_AFFINE;
      else if (fe_eq(fe_of(t.c0), p1)) how = PT_ONE;
      else if (fe_eq(fe_of(t.c0), m1)) how = PT_MINUS_ONE;
      a.terms[2 * e] = t.col;
      a.terms[2 * e + 1] = (uint32_t)t.kind | how << 8 | (uint32_t)t.c0 << 16 | (uint32_t)t.c1 << 24;
    }
    return Status{};
  });
  for (size_t k = 0; k < pr->n_consts; ++k) a.consts[k] = tape_val(&pr->consts[k]);
  a.rows = (uint32_t)rows;
  // the seven vectors of the cross term per row, and the gathered elements once (they are the repetitions' own variables)
  KTimer kt(s, "k_nifs_cross_periodic", (double)rows * 7 * 32 + (double)reps * pr->n_vars * 32);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_nifs_cross_periodic<tag_t<decltype(f)>>), grid_for(rows), dim3(256), 0, s, a, cbytes_of(o.z2), cbytes_of(o.abc1[0]),
                       cbytes_of(o.abc1[1]), cbytes_of(o.abc1[2]), tape_val(o.u1), bytes_of(o.abc2[0]), bytes_of(o.abc2[1]), bytes_of(o.abc2[2]),
                       bytes_of(o.T));
  });
}

}  // namespace vdf
