// libvdf_hip.so: MinRoot inverse walks (vdf_minroot_inverse_walk / vdf_minroot_check_batch) -- a step's forward trace rebuilt
// from the state it ends in.
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
