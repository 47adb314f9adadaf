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
#include "internal.h"
#include "fe.cuh"

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

template <class P>
__global__ __launch_bounds__(64) void k_round_tape(TapeArgs tape, const char* __restrict__ advice, uint64_t t, char* __restrict__ out) {
  extern __shared__ uint4 tape_slots[];
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint32_t lane = threadIdx.x;
  const uint64_t j = (uint64_t)blockIdx.x * 64 + lane;
  if (j >= t) return;
  const char* adv = advice + j * tape.n_adv * 32;
  char* o = out + j * tape.n_vars * 32;
  for (uint32_t i = 0; i < tape.n_ops; ++i) {
    const uint32_t w = tape.ops[i];
    const uint32_t op = w & 0xFF, dst = (w >> 8) & 0xFF, a = (w >> 16) & 0xFF, b = w >> 24;
    Fe<P> r;
    switch (op) {
      case VDF_TAPE_ADV: r = fe_load<P>(adv + (b * tape.n_adv + a) * 32); break;
      case VDF_TAPE_INV: r = tape_fe<P>(tape.inv[a]); break;
      case VDF_TAPE_J: r = fe_from_u64<P>(j); break;
      case VDF_TAPE_CONST: r = tape_fe<P>(tape.consts[a]); break;
      case VDF_TAPE_ADD: r = fe_add(slot_load<P>(tape_slots, a, lane), slot_load<P>(tape_slots, b, lane)); break;
      case VDF_TAPE_SUB: r = fe_sub(slot_load<P>(tape_slots, a, lane), slot_load<P>(tape_slots, b, lane)); break;
      case VDF_TAPE_MUL: {
        const Fe<P> x = slot_load<P>(tape_slots, a, lane);
        r = a == b ? fe_sqr(x) : fe_mul(x, slot_load<P>(tape_slots, b, lane));
        break;
      }
      case VDF_TAPE_SCALE: r = fe_mul(slot_load<P>(tape_slots, a, lane), tape_fe<P>(tape.consts[b])); break;
      default:                       // VDF_TAPE_OUT (the launcher admits no other opcode)
        fe_store<P>(o + b * 32, slot_load<P>(tape_slots, a, lane));
        continue;
    }
    slot_store<P>(tape_slots, dst, lane, r);
  }
}

// ---- walk tapes: the advice itself, rebuilt from checkpoints (vdf_hip.h vdf_round_tape_walk) ---------------------------------
// k_inverse_walk's launch (one lane per walk, workgroups of one wavefront, wave priority left at 0: background work beside a
// prover) around k_round_tape's interpreter.  Two entries of n_adv slots follow the value file in LDS: the one the walk stands on
// and the one the round produces, swapped on the round's parity -- an OUT to column c never touches what a later ADV of column c
// reads.  The slot numbers of both are scalars; nothing is indexed by a run-time value outside LDS.  A round is sequential after
// the one before it, so unlike k_round_tape the interpreter's scalar loads of the tape recur every round: they stay in the
// scalar cache (2.5 KiB of arguments).
struct WalkArgs {
  uint64_t n, walk_stride, top, group, group_stride, j_base, j_group_step;
  uint32_t rounds, n_slots, heads, pad;
};
static_assert(sizeof(TapeArgs) + sizeof(WalkArgs) + 32 <= 4096, "the tape travels in the kernel-argument segment");

template <class P>
__global__ __launch_bounds__(64) void k_tape_walk(TapeArgs tape, WalkArgs wa, char* __restrict__ entries, char* __restrict__ trace,
                                                  const char* __restrict__ expect, int32_t* __restrict__ ok) {
  extern __shared__ uint4 tape_slots[];
  const uint32_t lane = threadIdx.x;
  const uint64_t w = (uint64_t)blockIdx.x * 64 + lane;
  if (w >= wa.n) return;                             // (no barrier below: a lane touches only its own words of LDS)
  const uint32_t na = tape.n_adv;
  const size_t esz = (size_t)na * 32;
  char* const ep = entries + w * esz;
  const uint64_t g = w / wa.group, first = (w % wa.group) * wa.walk_stride + wa.top;      // local index of the entry the walk stands on
  uint32_t stand = wa.n_slots, prod = wa.n_slots + na;
  for (uint32_t c = 0; c < na; ++c) slot_store<P>(tape_slots, stand + c, lane, fe_load<P>(ep + c * 32));
  char* tp = trace ? trace + (g * wa.group_stride + first) * esz : nullptr;
  uint64_t j = wa.j_base + g * wa.j_group_step + first - 1;
#pragma unroll 1
  for (uint32_t r = 0; r < wa.rounds; ++r, --j) {
    if (tp) {
      for (uint32_t c = 0; c < na; ++c) fe_store<P>(tp + c * 32, slot_load<P>(tape_slots, stand + c, lane));
      tp -= esz;
    }
#pragma unroll 1
    for (uint32_t i = 0; i < tape.n_ops; ++i) {
      const uint32_t x = tape.ops[i];
      const uint32_t op = x & 0xFF, dst = (x >> 8) & 0xFF, a = (x >> 16) & 0xFF, b = x >> 24;
      Fe<P> v;
      switch (op) {
        case VDF_TAPE_ADV: v = slot_load<P>(tape_slots, stand + a, lane); break;      // (the launcher admits b = 1 only)
        case VDF_TAPE_INV: v = tape_fe<P>(tape.inv[a]); break;
        case VDF_TAPE_J: v = fe_from_u64<P>(j); break;
        case VDF_TAPE_CONST: v = tape_fe<P>(tape.consts[a]); break;
        case VDF_TAPE_ADD: v = fe_add(slot_load<P>(tape_slots, a, lane), slot_load<P>(tape_slots, b, lane)); break;
        case VDF_TAPE_SUB: v = fe_sub(slot_load<P>(tape_slots, a, lane), slot_load<P>(tape_slots, b, lane)); break;
        case VDF_TAPE_MUL: {
          const Fe<P> y = slot_load<P>(tape_slots, a, lane);
          v = a == b ? fe_sqr(y) : fe_mul(y, slot_load<P>(tape_slots, b, lane));
          break;
        }
        case VDF_TAPE_SCALE: v = fe_mul(slot_load<P>(tape_slots, a, lane), tape_fe<P>(tape.consts[b])); break;
        default:                       // VDF_TAPE_OUT
          slot_store<P>(tape_slots, prod + b, lane, slot_load<P>(tape_slots, a, lane));
          continue;
      }
      slot_store<P>(tape_slots, dst, lane, v);
    }
    const uint32_t t = stand; stand = prod; prod = t;
  }
  // where the walk landed: back into entries, to the head of its group's trace, and against the checkpoint
  uint32_t diff = 0;
  const bool head = tp && wa.heads && w % wa.group == 0;
  for (uint32_t c = 0; c < na; ++c) {
    const Fe<P> v = slot_load<P>(tape_slots, stand + c, lane);
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

// ---- forward walk tapes: the chain itself, many at once (vdf_hip.h vdf_round_tape_forward_walk) -------------------------------
// k_tape_walk ascending: the same launch (one lane per walk, workgroups of one wavefront, wave priority left at 0), the same
// interpreter and the same two entries behind the value file in LDS, swapped each round; what a round produces goes to the trace
// and, every `every` rounds, to the checkpoints, in k_forward_walk's layout.  The one new op is VDF_TAPE_POW: left-to-right
// square-and-multiply from the exponent's top set bit.  The base is read from its slot once and stays in registers with the
// accumulator; the exponent's words come from the kernel arguments by scalar loads, so the loop and the branch on every bit are
// wave-uniform.  No table, no LDS beyond the slots.
struct ForwardArgs {
  uint64_t n, walk_stride, cp_stride, every, base, j_base, j_walk_step;
  uint32_t rounds, n_slots;
};
static_assert(sizeof(TapeArgs) + sizeof(ForwardArgs) + 24 <= 4096, "the tape travels in the kernel-argument segment");

template <class P>
__global__ __launch_bounds__(64) void k_tape_forward_walk(TapeArgs tape, ForwardArgs fa, char* __restrict__ entries,
                                                          char* __restrict__ checkpoints, char* __restrict__ trace) {
  extern __shared__ uint4 tape_slots[];
  const uint32_t lane = threadIdx.x;
  const uint64_t w = (uint64_t)blockIdx.x * 64 + lane;
  if (w >= fa.n) return;                             // (no barrier below: a lane touches only its own words of LDS)
  const uint32_t na = tape.n_adv;
  const size_t esz = (size_t)na * 32;
  char* const ep = entries + w * esz;
  uint32_t stand = fa.n_slots, prod = fa.n_slots + na;
  for (uint32_t c = 0; c < na; ++c) slot_store<P>(tape_slots, stand + c, lane, fe_load<P>(ep + c * 32));
  // entry base + r + 1 after round r; checkpoint (base + r + 1) / every when `every` divides base + r + 1
  char* tp = trace ? trace + (w * fa.walk_stride + fa.base + 1) * esz : nullptr;
  uint64_t cp_left = checkpoints ? fa.every - fa.base % fa.every : 0;
  char* cp = checkpoints ? checkpoints + (w * fa.cp_stride + fa.base / fa.every + 1) * esz : nullptr;
  uint64_t j = fa.j_base + w * fa.j_walk_step + fa.base;
#pragma unroll 1
  for (uint32_t r = 0; r < fa.rounds; ++r, ++j) {
#pragma unroll 1
    for (uint32_t i = 0; i < tape.n_ops; ++i) {
      const uint32_t x = tape.ops[i];
      const uint32_t op = x & 0xFF, dst = (x >> 8) & 0xFF, a = (x >> 16) & 0xFF, b = x >> 24;
      Fe<P> v;
      switch (op) {
        case VDF_TAPE_ADV: v = slot_load<P>(tape_slots, stand + a, lane); break;      // (the launcher admits b = 0 only)
        case VDF_TAPE_INV: v = tape_fe<P>(tape.inv[a]); break;
        case VDF_TAPE_J: v = fe_from_u64<P>(j); break;
        case VDF_TAPE_CONST: v = tape_fe<P>(tape.consts[a]); break;
        case VDF_TAPE_ADD: v = fe_add(slot_load<P>(tape_slots, a, lane), slot_load<P>(tape_slots, b, lane)); break;
        case VDF_TAPE_SUB: v = fe_sub(slot_load<P>(tape_slots, a, lane), slot_load<P>(tape_slots, b, lane)); break;
        case VDF_TAPE_MUL: {
          const Fe<P> y = slot_load<P>(tape_slots, a, lane);
          v = a == b ? fe_sqr(y) : fe_mul(y, slot_load<P>(tape_slots, b, lane));
          break;
        }
        case VDF_TAPE_SCALE: v = fe_mul(slot_load<P>(tape_slots, a, lane), tape_fe<P>(tape.consts[b])); break;
        case VDF_TAPE_POW: {
          uint32_t q = 8, word = 0;                    // words of the exponent still to read, and the one being read
          while (q && (word = tape.consts[b].v[q - 1]) == 0) --q;
          if (q == 0) { v = fe_one<P>(); break; }      // E = 0
          const Fe<P> y = slot_load<P>(tape_slots, a, lane);
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
        default:                       // VDF_TAPE_OUT
          slot_store<P>(tape_slots, prod + b, lane, slot_load<P>(tape_slots, a, lane));
          continue;
      }
      slot_store<P>(tape_slots, dst, lane, v);
    }
    const uint32_t t = stand; stand = prod; prod = t;
    if (tp) {
      for (uint32_t c = 0; c < na; ++c) fe_store<P>(tp + c * 32, slot_load<P>(tape_slots, stand + c, lane));
      tp += esz;
    }
    if (cp && --cp_left == 0) {
      for (uint32_t c = 0; c < na; ++c) fe_store<P>(cp + c * 32, slot_load<P>(tape_slots, stand + c, lane));
      cp += esz;
      cp_left = fa.every;
    }
  }
  for (uint32_t c = 0; c < na; ++c) fe_store<P>(ep + c * 32, slot_load<P>(tape_slots, stand + c, lane));
}

static TapeFe tape_val(const vdf_fe* p) { TapeFe v; std::memcpy(&v, p, 32); return v; }
// what k_tape_forward_walk spends on a POW of exponent e: bitlen - 1 squarings and popcount - 1 products, at least one
static uint64_t pow_products(const TapeFe& e) {
  uint64_t bits = 0, ones = 0;
  for (int q = 0; q < 8; ++q)
    if (e.v[q]) { bits = 32 * q + 32 - __builtin_clz(e.v[q]); ones += __builtin_popcount(e.v[q]); }
  return bits + ones > 2 ? bits + ones - 2 : 1;
}

// Everything a tape could index out of range is checked here, before a launch: opcodes, slots against n_slots, columns,
// constants, invariants and variables against their counts, reads of slots nothing has written, variables written twice or never.
// TAPE_WALK / TAPE_FORWARD: the rules of a walk tape on top (vdf_hip.h): n_vars == n_adv, no ADV of the entry being produced
// (b = 0 descending, b = 1 ascending).  VDF_TAPE_POW is an op of forward tapes only.  products (if asked for): the field products of
// one round, a POW counted as its squarings and multiplications.
enum TapeMode { TAPE_ROUND, TAPE_WALK, TAPE_FORWARD };
static Status pack_tape(const vdf_round_tape* tp, const vdf_fe* inv, TapeMode mode, TapeArgs& a, uint64_t* products = nullptr) {
  const bool walk = mode != TAPE_ROUND;
  if (!tp || (tp->n_ops && !tp->ops) || (tp->n_consts && !tp->consts)) return Status{VDF_ERR_BAD_ARG, "null tape"};
  if (tp->n_ops > VDF_TAPE_MAX_OPS || tp->n_consts > VDF_TAPE_MAX_CONSTS || tp->n_slots > VDF_TAPE_MAX_SLOTS || tp->n_vars > VDF_TAPE_MAX_VARS ||
      tp->n_inv > VDF_TAPE_MAX_INV || tp->n_adv > VDF_TAPE_MAX_ADV || tp->n_vars == 0 || tp->n_adv == 0 || tp->n_slots == 0)
    return Status{VDF_ERR_BAD_ARG, "tape exceeds a published cap (VDF_TAPE_MAX_*), or has no variable, slot or advice column"};
  if (walk && tp->n_vars != tp->n_adv) return Status{VDF_ERR_BAD_ARG, "walk tape: n_vars != n_adv (a round writes one advice entry)"};
  if (tp->n_inv && !inv) return Status{VDF_ERR_BAD_ARG, "null inv"};
  std::memset(&a, 0, sizeof(a));
  a.n_ops = (uint32_t)tp->n_ops; a.n_vars = tp->n_vars; a.n_adv = tp->n_adv;
  bool written[VDF_TAPE_MAX_SLOTS] = {}, var_out[VDF_TAPE_MAX_VARS] = {};
  uint64_t n_products = 0;
  for (size_t i = 0; i < tp->n_ops; ++i) {
    const vdf_tape_op& o = tp->ops[i];
    auto slot_ok = [&](uint8_t x) { return x < tp->n_slots && written[x]; };
    bool ok = false;
    switch (o.op) {
      case VDF_TAPE_ADV: ok = o.a < tp->n_adv && (mode == TAPE_WALK ? o.b == 1 : mode == TAPE_FORWARD ? o.b == 0 : o.b <= 1); break;
      case VDF_TAPE_INV: ok = o.a < tp->n_inv; break;
      case VDF_TAPE_J: ok = true; break;
      case VDF_TAPE_CONST: ok = o.a < tp->n_consts; break;
      case VDF_TAPE_ADD: case VDF_TAPE_SUB: ok = slot_ok(o.a) && slot_ok(o.b); break;
      case VDF_TAPE_MUL: ok = slot_ok(o.a) && slot_ok(o.b); ++n_products; break;
      case VDF_TAPE_SCALE: ok = slot_ok(o.a) && o.b < tp->n_consts; ++n_products; break;
      case VDF_TAPE_OUT: ok = slot_ok(o.a) && o.b < tp->n_vars && !var_out[o.b]; if (ok) var_out[o.b] = true; break;
      case VDF_TAPE_POW:
        ok = mode == TAPE_FORWARD && slot_ok(o.a) && o.b < tp->n_consts;
        if (ok) n_products += pow_products(tape_val(&tp->consts[o.b]));
        break;
      default: break;
    }
    if (ok && o.op != VDF_TAPE_OUT) { ok = o.dst < tp->n_slots; if (ok) written[o.dst] = true; }
    if (!ok) return Status{VDF_ERR_BAD_ARG, "tape op " + std::to_string(i) + " is malformed (opcode, index out of range, or a slot read before it is written)" +
                                            (mode == TAPE_WALK ? "; a walk tape loads advice with b = 1 only" :
                                             mode == TAPE_FORWARD ? "; a forward walk tape loads advice with b = 0 only" : "")};
    a.ops[i] = (uint32_t)o.op | (uint32_t)o.dst << 8 | (uint32_t)o.a << 16 | (uint32_t)o.b << 24;
  }
  for (uint32_t v = 0; v < tp->n_vars; ++v)
    if (!var_out[v]) return Status{VDF_ERR_BAD_ARG, "tape leaves variable " + std::to_string(v) + " unwritten"};
  for (size_t k = 0; k < tp->n_consts; ++k) a.consts[k] = tape_val(&tp->consts[k]);
  for (uint32_t k = 0; k < tp->n_inv; ++k) a.inv[k] = tape_val(&inv[k]);
  if (products) *products = n_products ? n_products : 1;
  return Status{};
}

Status vec_round_tape(int field, const vdf_round_tape* tp, uint64_t t, const vdf_fe* inv, const void* advice, void* out, hipStream_t s) {
  TapeArgs a;
  VDF_TRY(pack_tape(tp, inv, TAPE_ROUND, a));
  // advice read + variables written per repetition
  KTimer kt(s, "k_round_tape", 32.0 * (tp->n_adv + tp->n_vars) * t);
  const dim3 grid((unsigned)((t + 63) / 64));
  const size_t lds = (size_t)tp->n_slots * 2 * 64 * sizeof(uint4);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_round_tape<tag_t<decltype(f)>>), grid, dim3(64), lds, s, a, cbytes_of(advice), t, bytes_of(out));
  });
}

Status vec_round_tape_walk(int field, const vdf_round_tape* tp, const vdf_fe* inv, void* entries, size_t n, uint64_t rounds, void* trace,
                           size_t walk_stride, size_t top, size_t group, size_t group_stride, uint64_t j_base, uint64_t j_group_step,
                           int heads, const void* expect, int32_t* ok, hipStream_t s) {
  VDF_TRY(check_field(field));
  TapeArgs a;
  VDF_TRY(pack_tape(tp, inv, TAPE_WALK, a));
  if (tp->n_slots + 2 * tp->n_adv > VDF_WALK_MAX_SLOTS)
    return Status{VDF_ERR_BAD_ARG, "walk tape: n_slots + 2 * n_adv > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)"};
  uint64_t products = 0;
  for (size_t i = 0; i < tp->n_ops; ++i) products += tp->ops[i].op == VDF_TAPE_MUL || tp->ops[i].op == VDF_TAPE_SCALE;
  if (products == 0) products = 1;
  if (rounds > VDF_WALK_MAX_WORK / products) return Status{VDF_ERR_BAD_ARG, "rounds x products per round > VDF_WALK_MAX_WORK in one call: cut the walk"};
  if (expect && !ok) return Status{VDF_ERR_BAD_ARG, "expect without ok"};
  if (n == 0 || rounds == 0) return Status{};
  if (n > ((size_t)1 << 31)) return Status{VDF_ERR_BAD_LENGTH, "more than 2^31 walks"};
  if (!entries) return Status{VDF_ERR_BAD_ARG, "null entries"};
  if (trace && top + 1 < rounds) return Status{VDF_ERR_BAD_ARG, "top < rounds - 1: the walk would write below its run"};
  if (trace && heads && top < rounds) return Status{VDF_ERR_BAD_ARG, "heads with top < rounds: the landing would be written below the run"};
  if (group == 0) { group = n; group_stride = 0; }
  WalkArgs wa;
  std::memset(&wa, 0, sizeof(wa));
  wa.n = n; wa.walk_stride = walk_stride; wa.top = top; wa.group = group; wa.group_stride = group_stride;
  wa.j_base = j_base; wa.j_group_step = j_group_step;
  wa.rounds = (uint32_t)rounds; wa.n_slots = tp->n_slots; wa.heads = heads != 0;
  KTimer kt(s, "k_tape_walk", trace ? 32.0 * tp->n_adv * (double)n * (double)rounds : 0.0);
  const size_t lds = (size_t)(tp->n_slots + 2 * tp->n_adv) * 2 * 64 * sizeof(uint4);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_tape_walk<tag_t<decltype(f)>>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, wa, bytes_of(entries),
                       bytes_of(trace), cbytes_of(expect), ok);
  });
}

// the forward-tape rules and the work cap, nothing launched: the rounds one call may run (vdf_round_tape_eval_batch cuts by it)
Status round_tape_forward_max_rounds(const vdf_round_tape* tp, const vdf_fe* inv, uint64_t* max_rounds) {
  TapeArgs a;
  uint64_t products = 1;
  VDF_TRY(pack_tape(tp, inv, TAPE_FORWARD, a, &products));
  if (tp->n_slots + 2 * tp->n_adv > VDF_WALK_MAX_SLOTS)
    return Status{VDF_ERR_BAD_ARG, "forward walk tape: n_slots + 2 * n_adv > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)"};
  *max_rounds = VDF_FORWARD_TAPE_MAX_WORK / products;
  return Status{};
}

Status vec_round_tape_forward_walk(int field, const vdf_round_tape* tp, const vdf_fe* inv, void* entries, size_t n, uint64_t rounds,
                                   void* checkpoints, uint64_t every, size_t cp_stride, void* trace, size_t walk_stride, uint64_t base,
                                   uint64_t j_base, uint64_t j_walk_step, hipStream_t s) {
  VDF_TRY(check_field(field));
  TapeArgs a;
  uint64_t products = 1;
  VDF_TRY(pack_tape(tp, inv, TAPE_FORWARD, a, &products));
  if (tp->n_slots + 2 * tp->n_adv > VDF_WALK_MAX_SLOTS)
    return Status{VDF_ERR_BAD_ARG, "forward walk tape: n_slots + 2 * n_adv > VDF_WALK_MAX_SLOTS (64 KiB of LDS per wavefront)"};
  if (rounds > VDF_FORWARD_TAPE_MAX_WORK / products)
    return Status{VDF_ERR_BAD_ARG, "rounds x products per round > VDF_FORWARD_TAPE_MAX_WORK in one call: cut the walk"};
  if (checkpoints && every == 0) return Status{VDF_ERR_BAD_ARG, "checkpoints without `every`"};
  if (n == 0 || rounds == 0) return Status{};
  if (n > ((size_t)1 << 31)) return Status{VDF_ERR_BAD_LENGTH, "more than 2^31 walks"};
  if (!entries) return Status{VDF_ERR_BAD_ARG, "null entries"};
  ForwardArgs fa;
  std::memset(&fa, 0, sizeof(fa));
  fa.n = n; fa.walk_stride = walk_stride; fa.cp_stride = cp_stride; fa.every = every; fa.base = base;
  fa.j_base = j_base; fa.j_walk_step = j_walk_step;
  fa.rounds = (uint32_t)rounds; fa.n_slots = tp->n_slots;
  KTimer kt(s, "k_tape_forward_walk", (trace ? 32.0 * tp->n_adv * (double)n * (double)rounds : 0.0) + 64.0 * tp->n_adv * (double)n);
  const size_t lds = (size_t)(tp->n_slots + 2 * tp->n_adv) * 2 * 64 * sizeof(uint4);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_tape_forward_walk<tag_t<decltype(f)>>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, a, fa, bytes_of(entries),
                       bytes_of(checkpoints), bytes_of(trace));
  });
}

}  // namespace vdf
