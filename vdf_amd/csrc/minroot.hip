// libvdf_hip.so: MinRoot walks, one lane per chain.  Inverse walks (vdf_minroot_inverse_walk / vdf_minroot_check_batch) -- a step's
// forward trace rebuilt from the state it ends in -- and forward walks (vdf_minroot_forward_walk / vdf_minroot_eval_batch) -- many
// chains evaluated at once (k_forward_walk below).
//
// The reference's round_inverse (src/minroot.rs:338-344) is (x, y, i) -> (y - (i - 1), x^5 - (y - (i - 1)), i - 1): two
// squarings, one product and three subtractions, against the ~285 dependent products of the forward round's fifth root, and
// it lands exactly on the state the forward round started from.  A walk is sequential in its rounds; walks are independent of
// each other -- one per step, or one per checkpoint interval of a step -- so a lane owns a walk.
//
// Shape of the launch: workgroups of ONE wavefront, so that a handful of walks spreads over CUs instead of stacking on one
// SIMD; no LDS; every value canonical after every operation, so that the stored (x, y) are byte for byte what the host's
// rounds give.  A lane stores 64 B per round at addresses `walk_stride` apart from its neighbours' (half a 128-B line each).
// Wave priority stays at the hardware's default of 0: this is background work beside a prover whose light kernels run at 3.
#include <cstring>
#include "internal.h"
#include "fe.cuh"
#include "minroot_chain.h"

namespace vdf {

template <class P>
__global__ __launch_bounds__(64) void k_inverse_walk(char* __restrict__ states, size_t n, uint32_t rounds, char* __restrict__ trace,
                                                     size_t walk_stride, size_t top, size_t group, size_t group_stride) {
  const size_t w = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= n) return;
  char* const sp = states + w * 96;
  Fe<P> x = fe_load<P>(sp), y = fe_load<P>(sp + 32), i = fe_load<P>(sp + 64);
  const Fe<P> one = fe_one<P>();
  // entry of the state the walk stands on; one entry (64 B) down per round
  char* tp = trace ? trace + 64 * ((w / group) * group_stride + (w % group) * walk_stride + top) : nullptr;
#pragma unroll 1
  for (uint32_t r = 0; r < rounds; ++r) {
    if (tp) {
      fe_store<P>(tp, x);
      fe_store<P>(tp + 32, y);
      tp -= 64;
    }
    i = fe_sub(i, one);
    const Fe<P> nx = fe_sub(y, i);
    const Fe<P> x5 = fe_mul_inl(x, fe_sqr_inl(fe_sqr_inl(x)));
    y = fe_sub(x5, nx);
    x = nx;
  }
  fe_store<P>(sp, x);
  fe_store<P>(sp + 32, y);
  fe_store<P>(sp + 64, i);
}

// ---- forward walks ----------------------------------------------------------------------------------------------------------
// The forward round (src/minroot.rs:329-335) is (x, y, i) -> ((x + y)^e, x + i, i + 1), e = 1/5 mod (m - 1): 253 squarings and 30
// (Fp: 29) products that each wait for the one before (minroot_chain.h), ~60,000 VALU instructions where the inverse round has ~700.  A
// chain cannot be spread over lanes without a cooperative product, so this is a THROUGHPUT kernel: a lane owns a
// chain, and it pays only when there are thousands of chains.  A lone chain is far slower here than on the host.
//
// Code size is the constraint: the chain inlined is ~280 products of ~1 KB each.  The kernel interprets the chain's program
// instead -- ONE squaring site, ONE product site, both in a loop whose trip counts come from the program through scalar loads
// (the program is the same for every lane, so every branch of the interpreter is wave-uniform).  The nine slots of the program
// are lane-private LDS, 9 x 32 B x 64 lanes = 18 KB per wavefront, laid out [slot][half][lane] in 16-byte words: a lane's
// ds_read_b128 / ds_write_b128 sit 16 B from its neighbours' (conflict-free), and the slot index is a scalar.  No register
// array is indexed dynamically and nothing spills.  8 wavefronts fit a CU's 160 KB: two per SIMD, the second covering the
// first's LDS round trips; the products themselves are dependent v_mad_u64_u32 that one wavefront already issues back to back.
//
// Inside a round the values are in the lazy domain of fe.cuh: squarings and products skip the conditional subtraction, each
// adds at most eps ~ 2^126 of slack to [0, 2m) -- below 2m + 283 eps < 2^256 at the chain's end -- and the result is made
// canonical once (fe_canon).  x, y, i are canonical at every round boundary, so states, checkpoints and trace entries are byte
// for byte what the host's vdf_minroot_round gives.
//
// Shape of the launch as k_inverse_walk's: workgroups of ONE wavefront, wave priority 0 (background work beside a prover).
__constant__ MinrootChainProgram c_minroot_chain[2] = {MINROOT_CHAIN_FP, MINROOT_CHAIN_FQ};
static_assert(VDF_FIELD_FP == 0 && VDF_FIELD_FQ == 1, "c_minroot_chain is indexed by the field");

template <class P>
__global__ __launch_bounds__(64) void k_forward_walk(char* __restrict__ states, size_t n, uint32_t rounds, char* __restrict__ checkpoints,
                                                     uint64_t every, size_t cp_stride, char* __restrict__ trace, size_t walk_stride,
                                                     uint64_t base) {
  __shared__ uint4 slot[MR_SLOTS * 2 * 64];
  const uint32_t lane = threadIdx.x;
  const size_t w = (size_t)blockIdx.x * 64 + lane;
  if (w >= n) return;                                      // (no barrier below: a lane touches only its own words of `slot`)
  const MinrootChainProgram& prog = c_minroot_chain[field_id(FieldTag<P>{})];
  char* const sp = states + w * 96;
  Fe<P> x = fe_load<P>(sp), y = fe_load<P>(sp + 32), i = fe_load<P>(sp + 64);
  const Fe<P> one = fe_one<P>();
  // entry base + r + 1 after round r; checkpoint (base + r + 1) / every when `every` divides base + r + 1
  char* tp = trace ? trace + 64 * (w * walk_stride + base + 1) : nullptr;
  uint64_t cp_left = checkpoints ? every - base % every : 0;
  char* cp = checkpoints ? checkpoints + 96 * (w * cp_stride + base / every + 1) : nullptr;
  auto put = [&](uint32_t s, const Fe<P>& a) {
    slot[(2 * s) * 64 + lane] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    slot[(2 * s + 1) * 64 + lane] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
  };
  auto get = [&](uint32_t s) {
    const uint4 lo = slot[(2 * s) * 64 + lane], hi = slot[(2 * s + 1) * 64 + lane];
    Fe<P> a;
    a.v[0] = lo.x; a.v[1] = lo.y; a.v[2] = lo.z; a.v[3] = lo.w;
    a.v[4] = hi.x; a.v[5] = hi.y; a.v[6] = hi.z; a.v[7] = hi.w;
    return a;
  };
#pragma unroll 1
  for (uint32_t r = 0; r < rounds; ++r) {
    Fe<P> v = fe_add(x, y);
    put(MR_S1, v);
#pragma unroll 1
    for (uint32_t k = 0; k < prog.len; ++k) {
      const MinrootChainStep st = prog.step[k];
      if (st.src != MR_ACC) v = get(st.src);
#pragma unroll 1
      for (uint32_t q = st.squarings; q; --q) v = fe_sqr_lazy(v);
      if (st.mul != MR_NONE) v = fe_mul_lazy(v, get(st.mul));
      if (st.dst != MR_NONE) put(st.dst, v);
    }
    y = fe_add(x, i);
    x = fe_canon(v);
    i = fe_add(i, one);
    if (tp) {
      fe_store<P>(tp, x);
      fe_store<P>(tp + 32, y);
      tp += 64;
    }
    if (cp && --cp_left == 0) {
      fe_store<P>(cp, x);
      fe_store<P>(cp + 32, y);
      fe_store<P>(cp + 64, i);
      cp += 96;
      cp_left = every;
    }
  }
  fe_store<P>(sp, x);
  fe_store<P>(sp + 32, y);
  fe_store<P>(sp + 64, i);
}

// ok[w] = 1 iff the 96 bytes of a[w] and b[w] are equal
__global__ __launch_bounds__(64) void k_states_match(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n,
                                                     int* __restrict__ ok) {
  const size_t w = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= n) return;
  uint32_t d = 0;
#pragma unroll
  for (int j = 0; j < 24; ++j) d |= a[w * 24 + j] ^ b[w * 24 + j];
  ok[w] = d == 0;
}

// entry 0 of trace k = (x, y) of states[k * state_stride]
__global__ __launch_bounds__(64) void k_trace_heads(const uint4* __restrict__ states, size_t n, size_t state_stride,
                                                    uint4* __restrict__ trace, size_t trace_stride) {
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  const uint4* s = states + k * state_stride * 6;      // 96 B = 6 x 16
  uint4* t = trace + k * trace_stride * 4;             // 64 B = 4 x 16
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = s[j];
}

static dim3 waves_for(size_t n) { return dim3((unsigned)((n + 63) / 64)); }

Status minroot_inverse_walk(int field, void* states, size_t n, uint64_t rounds, void* trace, size_t walk_stride, size_t top,
                            size_t group, size_t group_stride, hipStream_t s) {
  VDF_TRY(check_field(field));
  if (n == 0 || rounds == 0) return Status{};
  if (rounds > MINROOT_WALK_MAX_ROUNDS) return Status{VDF_ERR_BAD_ARG, "more than 2^22 rounds in one call: cut the walk"};
  if (n > ((size_t)1 << 31)) return Status{VDF_ERR_BAD_LENGTH, "more than 2^31 walks"};
  if (trace && top + 1 < rounds) return Status{VDF_ERR_BAD_ARG, "top < rounds - 1: the walk would write below its run"};
  if (group == 0) { group = n; group_stride = 0; }
  KTimer kt(s, "k_inverse_walk", trace ? 64.0 * (double)n * (double)rounds : 0.0);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_inverse_walk<tag_t<decltype(f)>>), waves_for(n), dim3(64), 0, s, bytes_of(states), n, (uint32_t)rounds,
                       bytes_of(trace), walk_stride, top, group, group_stride);
  });
}

Status minroot_forward_walk(int field, void* states, size_t n, uint64_t rounds, void* checkpoints, uint64_t every, size_t cp_stride,
                            void* trace, size_t walk_stride, uint64_t base, hipStream_t s) {
  VDF_TRY(check_field(field));
  if (rounds > VDF_MINROOT_FORWARD_MAX_ROUNDS) return Status{VDF_ERR_BAD_ARG, "more than VDF_MINROOT_FORWARD_MAX_ROUNDS rounds in one call: cut the walk"};
  if (n > ((size_t)1 << 31)) return Status{VDF_ERR_BAD_LENGTH, "more than 2^31 walks"};
  if (checkpoints && every == 0) return Status{VDF_ERR_BAD_ARG, "checkpoints without `every`"};
  if (n == 0 || rounds == 0) return Status{};
  KTimer kt(s, "k_forward_walk", (trace ? 64.0 * (double)n * (double)rounds : 0.0) + 192.0 * (double)n);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_forward_walk<tag_t<decltype(f)>>), waves_for(n), dim3(64), 0, s, bytes_of(states), n, (uint32_t)rounds,
                       bytes_of(checkpoints), every, cp_stride, bytes_of(trace), walk_stride, base);
  });
}

Status minroot_states_match(const void* a, const void* b, size_t n, int* ok, hipStream_t s) {
  if (n == 0) return Status{};
  KTimer kt(s, "k_states_match", 0.0);
  hipLaunchKernelGGL(k_states_match, waves_for(n), dim3(64), 0, s, (const uint32_t*)a, (const uint32_t*)b, n, ok);
  VDF_TRY_HIP(hipGetLastError());
  return Status{};
}

Status minroot_trace_heads(const void* states, size_t n, size_t state_stride, void* trace, size_t trace_stride, hipStream_t s) {
  if (n == 0) return Status{};
  KTimer kt(s, "k_trace_heads", 0.0);
  hipLaunchKernelGGL(k_trace_heads, waves_for(n), dim3(64), 0, s, (const uint4*)states, n, state_stride, (uint4*)trace, trace_stride);
  VDF_TRY_HIP(hipGetLastError());
  return Status{};
}

}  // namespace vdf
