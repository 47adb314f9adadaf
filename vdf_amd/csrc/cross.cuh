// The NIFS cross term of a running instance (A z1, B z1, C z1, u1) and a FRESH one (u2 = 1),
//   T = Az1 o Bz2 + Az2 o Bz1 - u1 Cz2 - Cz1,
// and the small pieces the kernels that compute it share (vecops.hip, rounds.hip).  Everything here is inlined into a kernel that
// keeps its own __restrict__ pointer parameters: no pointer is declared here as anything the kernel did not say itself.
#pragma once
#include "fe.cuh"

namespace vdf {

template <class P>
__device__ __forceinline__ Fe<P> cross_value(const Fe<P>& a1, const Fe<P>& b1, const Fe<P>& c1, const Fe<P>& u1, const Fe<P>& a2,
                                             const Fe<P>& b2, const Fe<P>& c2) {
  Fe<P> t = fe_add(fe_mul(a1, b2), fe_mul(a2, b1));
  t = fe_sub(t, fe_mul(u1, c2));
  return fe_sub(t, c1);
}

// How every cross-term kernel ends row r: the fresh A z2, B z2, C z2 stored on the way, then T.
template <class P>
__device__ __forceinline__ void cross_finish(char* az2, char* bz2, char* cz2, char* T, size_t r, const Fe<P>& a1, const Fe<P>& b1,
                                             const Fe<P>& c1, const Fe<P>& u1, const Fe<P>& a2, const Fe<P>& b2, const Fe<P>& c2) {
  fe_store<P>(az2 + r * 32, a2);
  fe_store<P>(bz2 + r * 32, b2);
  fe_store<P>(cz2 + r * 32, c2);
  const Fe<P> t = cross_value(a1, b1, c1, u1, a2, b2, c2);
  fe_store<P>(T + r * 32, t);
}

// Montgomery form of a round counter: below 2^30 without a Montgomery product (fe.cuh fe_from_small)
template <class P> __device__ __forceinline__ Fe<P> fe_from_count(uint64_t k) {
  return k < (1u << 30) ? fe_from_small<P>((uint32_t)k) : fe_from_u64<P>(k);
}

// k * z2[one] in a stencil row.  unit: the constant's value is ONE, as in every fresh instance (the same for all lanes: a uniform
// branch), and then the conversion is all it takes.
template <class P> __device__ __forceinline__ Fe<P> times_one(uint64_t k, bool unit, const Fe<P>& onev) {
  const Fe<P> km = fe_from_count<P>(k);
  return unit ? km : fe_mul(km, onev);
}

// The sum of `a` over each aligned group of LANES lanes of a wavefront (a power of two up to 64), in every lane of the group: a
// butterfly of log2 LANES steps, the farthest partner first.
template <class P, int LANES>
__device__ __forceinline__ Fe<P> fe_group_sum(Fe<P> a) {
#pragma unroll
  for (int off = LANES / 2; off >= 1; off >>= 1) {
    Fe<P> o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o.v[i] = __shfl_xor(a.v[i], off, 64);
    a = fe_add(a, o);
  }
  return a;
}

}  // namespace vdf
