// Field-vector kernels of the Nova folding step for gfx950 (all HBM-streaming, one element per lane,
// 2 x dwordx4 per 32-byte element; a wave touches 2 KiB of contiguous memory per operand).
//
// Replaces, on the prove_step path (/root/reference/src/nova/proof.rs:342-349 -> nova-snark 0.8.0):
//   k_axpy            RelaxedR1CSWitness::fold   W1 + r*W2, E1 + r*T            
//   k_cross_term      NIFS::prove / commit_T     AZ1*BZ2 + AZ2*BZ1 - u1*CZ2 - CZ1 (K5, a14)
//   k_spmv            R1CSShape::multiply_vec    Az, Bz, Cz (CSR, coefficient dictionary) (K4, a13)
//   k_minroot_witness InverseMinRootCircuit::synthesize / inverse_round witness values
//                     (/root/reference/src/nova/proof.rs:107-126, :162-189)          (K7, a1/a2)
#include <cstring>
#include "internal.h"
#include "fe.cuh"
#include "cross.cuh"

namespace vdf {


template <class P>
__global__ __launch_bounds__(256) void k_axpy(const char* __restrict__ a, const char* __restrict__ r,
                                              const char* __restrict__ b, size_t n, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Fe<P> rr = fe_load<P>(r);
  Fe<P> x = fe_load<P>(a + i * 32);
  Fe<P> y = fe_load<P>(b + i * 32);
  fe_store<P>(out + i * 32, fe_add(x, fe_mul(rr, y)));
}

template <class P>
__global__ __launch_bounds__(256) void k_cross_term(const char* __restrict__ az1, const char* __restrict__ bz1,
                                                    const char* __restrict__ cz1, const char* __restrict__ az2,
                                                    const char* __restrict__ bz2, const char* __restrict__ cz2,
                                                    const char* __restrict__ u1, size_t n, char* __restrict__ T) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Fe<P> u = fe_load<P>(u1);
  Fe<P> a1 = fe_load<P>(az1 + i * 32), b1 = fe_load<P>(bz1 + i * 32), c1 = fe_load<P>(cz1 + i * 32);
  Fe<P> a2 = fe_load<P>(az2 + i * 32), b2 = fe_load<P>(bz2 + i * 32), c2 = fe_load<P>(cz2 + i * 32);
  const Fe<P> t = cross_value(a1, b1, c1, u, a2, b2, c2);
  fe_store<P>(T + i * 32, t);
}

// Round j (0-based) of the inverse walk starts from forward state t-j and lands on t-j-1:
//   new_x = x_{t-j-1}, tmp1 = x_{t-j}^2, tmp2 = tmp1^2, new_y = y_{t-j-1}
// (new_x = y - (i-1) and new_y = x^5 - new_x of src/nova/proof.rs:167-189 are exactly the previous
// forward state, src/minroot.rs:329-344).  Thread t writes final_i = i0.
template <class P>
__global__ __launch_bounds__(256) void k_minroot_witness(const char* __restrict__ trace, const char* __restrict__ i0,
                                                         uint64_t t, char* __restrict__ W) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j > t) return;
  if (j == t) {
    fe_store<P>(W + 4 * t * 32, fe_load<P>(i0));
    return;
  }
  const Fe<P> x = fe_load<P>(trace + (t - j) * 64);
  const Fe<P> nx = fe_load<P>(trace + (t - j - 1) * 64);
  const Fe<P> ny = fe_load<P>(trace + (t - j - 1) * 64 + 32);
  const Fe<P> t1 = fe_sqr(x);
  const Fe<P> t2 = fe_sqr(t1);
  char* o = W + j * 128;
  fe_store<P>(o, nx);
  fe_store<P>(o + 32, t1);
  fe_store<P>(o + 64, t2);
  fe_store<P>(o + 96, ny);
}

// CSR sparse mat-vec; coefficient index 0 means +1 and 1 means -1 (no multiply), anything else
// indexes the dictionary.  One row per lane: R1CS rows are short (1-4 entries) and uniform.
template <class P>
__global__ __launch_bounds__(256) void k_spmv(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col,
                                              const uint32_t* __restrict__ coef, const char* __restrict__ dict,
                                              const char* __restrict__ z, size_t rows, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const uint32_t lo = rowptr[r], hi = rowptr[r + 1];
  if (hi - lo > VDF_LONG_ROW) return;                  // summed by a wavefront already (k_spmv_long)
  Fe<P> acc = fe_zero<P>();
  for (uint32_t k = lo; k < hi; ++k) {
    const Fe<P> v = fe_load<P>(z + (size_t)col[k] * 32);
    const uint32_t ci = coef[k];
    if (ci == 0) acc = fe_add(acc, v);
    else if (ci == 1) acc = fe_sub(acc, v);
    else acc = fe_add(acc, fe_mul(v, fe_load<P>(dict + (size_t)ci * 32)));
  }
  fe_store<P>(out + r * 32, acc);
}

// ---- fused NIFS step kernels: one launch per stage of a fold, small operands by value ---------------------
struct FeVal { uint32_t v[8]; };                      // a field element as a kernel argument
struct StepConsts { FeVal z_in[3], i0, u, X[6]; };    // everything of a fresh z that is not a round value
template <class P> __device__ __forceinline__ Fe<P> fe_from_val(const FeVal& a) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = a.v[i];
  return r;
}

// z = [ z_in(3) | per round new_x, tmp1, tmp2, new_y (4t) | final_i | u | X(6) ]: the whole fresh column vector
// of the exposed-IO step circuit; round values as in k_minroot_witness, the rest from kernel arguments.
// `packed` (optional): the same witness without the new_x values, [ z_in(3) | per round tmp1, tmp2, new_y (3t) |
// final_i ] -- new_x of a round is an affine image of another witness value, so a commitment needs no term for it
// (vdf_minroot_step_z_packed).
template <class P>
__global__ __launch_bounds__(256) void k_step_z(const char* __restrict__ trace, StepConsts k, uint64_t t,
                                                char* __restrict__ z, char* __restrict__ packed) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j > t) return;
  if (j == t) {
    for (int i = 0; i < 3; ++i) fe_store<P>(z + i * 32, fe_from_val<P>(k.z_in[i]));
    char* tail = z + (3 + 4 * t) * 32;
    fe_store<P>(tail, fe_from_val<P>(k.i0));
    fe_store<P>(tail + 32, fe_from_val<P>(k.u));
    for (int i = 0; i < 6; ++i) fe_store<P>(tail + 64 + i * 32, fe_from_val<P>(k.X[i]));
    if (packed) {
      for (int i = 0; i < 3; ++i) fe_store<P>(packed + i * 32, fe_from_val<P>(k.z_in[i]));
      fe_store<P>(packed + (3 + 3 * t) * 32, fe_from_val<P>(k.i0));
    }
    return;
  }
  const Fe<P> x = fe_load<P>(trace + (t - j) * 64);
  const Fe<P> nx = fe_load<P>(trace + (t - j - 1) * 64);
  const Fe<P> ny = fe_load<P>(trace + (t - j - 1) * 64 + 32);
  const Fe<P> t1 = fe_sqr(x);
  const Fe<P> t2 = fe_sqr(t1);
  char* o = z + 96 + j * 128;
  fe_store<P>(o, nx);
  fe_store<P>(o + 32, t1);
  fe_store<P>(o + 64, t2);
  fe_store<P>(o + 96, ny);
  if (packed) {
    char* q = packed + 96 + j * 96;
    fe_store<P>(q, t1);
    fe_store<P>(q + 32, t2);
    fe_store<P>(q + 64, ny);
  }
}

// The variables InverseMinRootCircuit::synthesize allocates inside an augmented circuit (no z_in, u, X around them):
// per round [new_x,] tmp1, tmp2, new_y, then final_i.  per = 4 is the reference's allocation (src/nova/proof.rs:167-181),
// per = 3 the bound form without new_x (oracle/nova.py InverseMinRootCircuit).
template <class P>
__global__ __launch_bounds__(256) void k_step_segment(const char* __restrict__ trace, FeVal i0, uint64_t t, int per,
                                                      char* __restrict__ out, char* __restrict__ packed, FeVal i_in) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j > t) return;
  if (j == t) {
    fe_store<P>(out + (size_t)per * t * 32, fe_from_val<P>(i0));
    if (packed) {                    // [3t] final_i, [3t + 1] y of the first round, [3t + 2] i of the first round, [3t + 3] one
      char* q = packed + (size_t)3 * t * 32;
      fe_store<P>(q, fe_from_val<P>(i0));
      fe_store<P>(q + 32, fe_load<P>(trace + t * 64 + 32));
      fe_store<P>(q + 64, fe_from_val<P>(i_in));
      fe_store<P>(q + 96, fe_one<P>());
    }
    return;
  }
  const Fe<P> x = fe_load<P>(trace + (t - j) * 64);
  const Fe<P> t1 = fe_sqr(x);
  const Fe<P> t2 = fe_sqr(t1);
  const Fe<P> ny = fe_load<P>(trace + (t - j - 1) * 64 + 32);
  char* o = out + j * (size_t)per * 32;
  if (per == 4) { fe_store<P>(o, fe_load<P>(trace + (t - j - 1) * 64)); o += 32; }
  fe_store<P>(o, t1);
  fe_store<P>(o + 32, t2);
  fe_store<P>(o + 64, ny);
  if (packed) {
    char* q = packed + j * 96;
    fe_store<P>(q, t1);
    fe_store<P>(q + 32, t2);
    fe_store<P>(q + 64, ny);
  }
}

// The variables LanesForwardCircuit::synthesize allocates (oracle/nova.py's primary= seam; include/vdf_nova.h
// VDF_CIRCUIT_MINROOT_FORWARD and _LANES), lane after lane: per round x_(j+1) -- the fifth root, taken from the forward trace -- and
// its square and fourth power, then final_i = i_end.  A trace is read in the direction it was written: round j reads entry j + 1.
// Lane l = blockIdx.y reads the trace that starts lane_stride entries after lane l - 1's and writes its 3t + 1 variables behind
// lane l - 1's; a single chain is the launch of one lane.  The lanes' last round counters arrive as kernel arguments (no
// staging copy): the lane picks its own with a uniform index.
struct LaneEnds { FeVal v[VDF_MINROOT_MAX_LANES]; };
template <class P>
__global__ __launch_bounds__(256) void k_forward_segment_lanes(const char* __restrict__ trace, size_t lane_stride, LaneEnds i_end,
                                                               uint64_t t, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint32_t lane = blockIdx.y;
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j > t) return;
  char* lo = out + (size_t)lane * (3 * t + 1) * 32;
  if (j == t) {
    fe_store<P>(lo + (size_t)3 * t * 32, fe_from_val<P>(i_end.v[lane]));
    return;
  }
  const Fe<P> x = fe_load<P>(trace + ((size_t)lane * lane_stride + j + 1) * 64);
  const Fe<P> t1 = fe_sqr(x);
  const Fe<P> t2 = fe_sqr(t1);
  char* o = lo + j * 96;
  fe_store<P>(o, x);
  fe_store<P>(o + 32, t1);
  fe_store<P>(o + 64, t2);
}

struct Csr3 { const uint32_t* rowptr[3]; const uint32_t* col[3]; const uint32_t* coef[3]; };

// One term of a sparse row: +-z[col] or coefficient * z[col] (dictionary index 0 = +1, 1 = -1).
template <class P>
__device__ __forceinline__ Fe<P> spmv_term(const Fe<P>& v, uint32_t ci, const char* __restrict__ dict) {
  if (ci == 0) return v;
  if (ci == 1) return fe_neg(v);
  return fe_mul(v, fe_load<P>(dict + (size_t)ci * 32));
}

// Rows of more than VDF_LONG_ROW entries, one wavefront each: lanes stride over the entries, then a butterfly sum.
template <class P>
__global__ __launch_bounds__(256) void k_spmv_long(Csr3 m, const char* __restrict__ dict, const char* __restrict__ z,
                                                   const uint32_t* __restrict__ long_rows, size_t n_long, char* __restrict__ o0,
                                                   char* __restrict__ o1, char* __restrict__ o2) {
  __builtin_amdgcn_s_setprio(3);
  const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_long) return;                                          // whole wavefronts leave together
  const uint32_t lane = threadIdx.x & 63, packed = long_rows[w], k = packed >> 30, r = packed & 0x3FFFFFFFu;
  const uint32_t* rowptr = k == 0 ? m.rowptr[0] : (k == 1 ? m.rowptr[1] : m.rowptr[2]);
  const uint32_t* col = k == 0 ? m.col[0] : (k == 1 ? m.col[1] : m.col[2]);
  const uint32_t* coef = k == 0 ? m.coef[0] : (k == 1 ? m.coef[1] : m.coef[2]);
  char* out = k == 0 ? o0 : (k == 1 ? o1 : o2);
  const uint32_t lo = rowptr[r], hi = rowptr[r + 1];
  Fe<P> acc = fe_zero<P>();
  for (uint32_t e = lo + lane; e < hi; e += 64)
    acc = fe_add(acc, spmv_term<P>(fe_load<P>(z + (size_t)col[e] * 32), coef[e], dict));
  acc = fe_group_sum<P, 64>(acc);
  if (lane == 0) fe_store<P>(out + (size_t)r * 32, acc);
}

// multiply_vec(z2) and the cross term in one pass over the rows:
//   (a2, b2, c2) = (A z2, B z2, C z2)[row];  T[row] = a1*b2 + a2*b1 - u1*c2 - c1      (u2 = 1)
// The loads are issued in three waves instead of nine dependent steps: all six row pointers, then the first column /
// coefficient of each matrix, then the three z values (R1CS rows are short: the first entry is usually the only one);
// the remaining entries of a row follow in a plain loop.
template <class P>
__global__ __launch_bounds__(256) void k_nifs_cross(Csr3 m, const char* __restrict__ dict, const char* __restrict__ z2,
                                                    const char* __restrict__ az1, const char* __restrict__ bz1,
                                                    const char* __restrict__ cz1, FeVal u1, size_t rows,
                                                    size_t skip_begin, size_t skip_len,
                                                    char* __restrict__ az2, char* __restrict__ bz2,
                                                    char* __restrict__ cz2, char* __restrict__ T) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  if (r >= skip_begin) r += skip_len;  // `rows` rows of the matrix, leaving out [skip_begin, skip_begin + skip_len)
  uint32_t lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = m.rowptr[k][r]; hi[k] = m.rowptr[k][r + 1]; }
  const Fe<P> a1 = fe_load<P>(az1 + r * 32), b1 = fe_load<P>(bz1 + r * 32), c1 = fe_load<P>(cz1 + r * 32);
  // Loads in three waves instead of one dependent round trip per entry: the row pointers; then column and coefficient of
  // the first PRE[k] entries of each matrix (a MinRoot row is 1 + 1 + at most 4 entries: src/nova/proof.rs:219-227); then
  // all their z values at once.  Entries past PRE[k] (rows of the augmented circuit, at most VDF_LONG_ROW) follow in a loop.
  constexpr int PRE[3] = {2, 2, 4};
  uint32_t cc[3][4], kk[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < PRE[k]; ++j) {
      const uint32_t e = lo[k] + j < hi[k] ? lo[k] + j : lo[k];       // (arrays are nnz + 1 long: lo is always readable)
      cc[k][j] = m.col[k][e];
      kk[k][j] = m.coef[k][e];
    }
  Fe<P> v[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < PRE[k]; ++j) v[k][j] = fe_load<P>(z2 + (size_t)(lo[k] + j < hi[k] ? cc[k][j] : 0u) * 32);
  Fe<P> acc[3];
  char* const outs[3] = {az2, bz2, cz2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (hi[k] - lo[k] > VDF_LONG_ROW) { acc[k] = fe_load<P>(outs[k] + r * 32); continue; }      // k_spmv_long ran first
    acc[k] = hi[k] > lo[k] ? spmv_term<P>(v[k][0], kk[k][0], dict) : fe_zero<P>();
#pragma unroll
    for (int j = 1; j < PRE[k]; ++j)
      if (lo[k] + j < hi[k]) acc[k] = fe_add(acc[k], spmv_term<P>(v[k][j], kk[k][j], dict));
    for (uint32_t e = lo[k] + PRE[k]; e < hi[k]; ++e)
      acc[k] = fe_add(acc[k], spmv_term<P>(fe_load<P>(z2 + (size_t)m.col[k][e] * 32), m.coef[k][e], dict));
  }
  cross_finish<P>(az2, bz2, cz2, T, r, a1, b1, c1, fe_from_val<P>(u1), acc[0], acc[1], acc[2]);
}

// The same with LPR lanes per row (4 or 8): lane l of a row's group takes the entries l, l + LPR, ... of each of the three
// sparse rows, so that all gathers of a row are in flight at once instead of one dependent round trip per entry, and a
// butterfly over the group's lanes (log2 LPR steps) adds the terms up; the group's first lane finishes the cross term.
// What it buys is LATENCY: the ~10^4 rows of an augmented circuit that a step waits for take 12 us instead of 26-48 (a lane
// that walks 8 entries of 3 matrices in turn pays 24 round trips); for the 2 x 10^5 uniform rows of the MinRoot rounds
// (1 + 1 + 4 entries) four lanes per row issue the four gathers of C together.
// (LEAVE_LONG: a row with a matrix of more than VDF_LONG_ROW entries is left to the wavefront k_nifs_cross_f gives it)
template <class P, int LPR, bool LEAVE_LONG>
__device__ __forceinline__ void nifs_cross_group(const Csr3& m, const char* __restrict__ dict, const char* __restrict__ z2,
                                                 const char* __restrict__ az1, const char* __restrict__ bz1,
                                                 const char* __restrict__ cz1, const FeVal& u1, size_t rows, size_t skip_begin,
                                                 size_t skip_len, char* __restrict__ az2, char* __restrict__ bz2,
                                                 char* __restrict__ cz2, char* __restrict__ T, uint32_t block) {
  constexpr uint32_t RPB = 256 / LPR;                                // rows per workgroup
  const uint32_t l = threadIdx.x & (LPR - 1);
  size_t r = (size_t)block * RPB + threadIdx.x / LPR;
  bool live = r < rows;
  if (!live) r = rows ? rows - 1 : 0;                                // keeps the group's lanes together for the butterfly
  if (r >= skip_begin) r += skip_len;
  uint32_t lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = m.rowptr[k][r]; hi[k] = m.rowptr[k][r + 1]; }
  if (LEAVE_LONG && (hi[0] - lo[0] > VDF_LONG_ROW || hi[1] - lo[1] > VDF_LONG_ROW || hi[2] - lo[2] > VDF_LONG_ROW)) {
    live = false;                                                    // (all lanes of the group agree: the row is theirs)
    hi[0] = lo[0]; hi[1] = lo[1]; hi[2] = lo[2];
  }
  Fe<P> a1, b1, c1;
  if (l == 0) { a1 = fe_load<P>(az1 + r * 32); b1 = fe_load<P>(bz1 + r * 32); c1 = fe_load<P>(cz1 + r * 32); }
  char* const outs[3] = {az2, bz2, cz2};
  Fe<P> acc[3], v[3];
  uint32_t cc[3], kk[3];
  bool has[3], longrow[3];
  // every lane's first entry of each matrix: column and coefficient of all three issued together, then the three gathers
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    longrow[k] = hi[k] - lo[k] > VDF_LONG_ROW;
    has[k] = !longrow[k] && lo[k] + l < hi[k];
    const uint32_t e = has[k] ? lo[k] + l : lo[k];                   // (arrays are nnz + 1 long: lo is always readable)
    cc[k] = m.col[k][e];
    kk[k] = m.coef[k][e];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = fe_load<P>(z2 + (size_t)(has[k] ? cc[k] : 0u) * 32);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    acc[k] = has[k] ? spmv_term<P>(v[k], kk[k], dict) : fe_zero<P>();
    if (longrow[k]) { if (l == 0) acc[k] = fe_load<P>(outs[k] + r * 32); continue; }       // k_spmv_long ran first
    for (uint32_t e = lo[k] + l + LPR; e < hi[k]; e += LPR)
      acc[k] = fe_add(acc[k], spmv_term<P>(fe_load<P>(z2 + (size_t)m.col[k][e] * 32), m.coef[k][e], dict));
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = fe_group_sum<P, LPR>(acc[k]);
  if (l != 0 || !live) return;
  cross_finish<P>(az2, bz2, cz2, T, r, a1, b1, c1, fe_from_val<P>(u1), acc[0], acc[1], acc[2]);
}

template <class P, int LPR>
__global__ __launch_bounds__(256) void k_nifs_cross_w(Csr3 m, const char* __restrict__ dict, const char* __restrict__ z2,
                                                      const char* __restrict__ az1, const char* __restrict__ bz1,
                                                      const char* __restrict__ cz1, FeVal u1, size_t rows,
                                                      size_t skip_begin, size_t skip_len,
                                                      char* __restrict__ az2, char* __restrict__ bz2,
                                                      char* __restrict__ cz2, char* __restrict__ T) {
  __builtin_amdgcn_s_setprio(3);
  nifs_cross_group<P, LPR, false>(m, dict, z2, az1, bz1, cz1, u1, rows, skip_begin, skip_len, az2, bz2, cz2, T, blockIdx.x);
}

// The cross term of an augmented circuit in ONE launch instead of k_spmv_long followed by k_nifs_cross_w: the first
// `long_wgs` workgroups give every row that has a matrix of more than VDF_LONG_ROW entries (the S-box rows of the
// circuit's hash: sums of a few hundred terms) a wavefront of its own, the others run the eight-lane groups over all rows
// and leave those rows alone.  A step waits for this kernel with the device otherwise idle on its queue, so what counts is
// its depth in dependent memory round trips, not its work: a long row is the list entry, the six row pointers, then per
// pass of 128 entries the column / coefficient indices of all three matrices, then their z and dictionary values -- every
// load of a pass is in flight before the first product (two passes cover the longest rows of the built-in circuits).
template <class P>
__global__ __launch_bounds__(256) void k_nifs_cross_f(Csr3 m, const char* __restrict__ dict, const char* __restrict__ z2,
                                                      const char* __restrict__ az1, const char* __restrict__ bz1,
                                                      const char* __restrict__ cz1, FeVal u1, size_t rows,
                                                      size_t skip_begin, size_t skip_len,
                                                      const uint32_t* __restrict__ long_rowlist, size_t n_long_rows,
                                                      uint32_t long_wgs, char* __restrict__ az2, char* __restrict__ bz2,
                                                      char* __restrict__ cz2, char* __restrict__ T) {
  __builtin_amdgcn_s_setprio(3);
  if (blockIdx.x >= long_wgs) {
    nifs_cross_group<P, 8, true>(m, dict, z2, az1, bz1, cz1, u1, rows, skip_begin, skip_len, az2, bz2, cz2, T,
                                 blockIdx.x - long_wgs);
    return;
  }
  const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_long_rows) return;                                     // whole wavefronts leave together
  const uint32_t lane = threadIdx.x & 63;
  const size_t r = long_rowlist[w];
  uint32_t lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = m.rowptr[k][r]; hi[k] = m.rowptr[k][r + 1]; }
  Fe<P> a1, b1, c1;
  if (lane == 0) { a1 = fe_load<P>(az1 + r * 32); b1 = fe_load<P>(bz1 + r * 32); c1 = fe_load<P>(cz1 + r * 32); }
  uint32_t longest = hi[0] - lo[0];
  if (hi[1] - lo[1] > longest) longest = hi[1] - lo[1];
  if (hi[2] - lo[2] > longest) longest = hi[2] - lo[2];
  Fe<P> acc[3] = {fe_zero<P>(), fe_zero<P>(), fe_zero<P>()};
  for (uint32_t base = 0; base < longest; base += 128) {            // (the same trip count for every lane of the wavefront)
    uint32_t cc[3][2], kk[3][2];
    bool has[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t e = lo[k] + base + lane + 64 * j;
        has[k][j] = e < hi[k];
        cc[k][j] = m.col[k][has[k][j] ? e : lo[k]];                   // (arrays are nnz + 1 long: lo is always readable)
        kk[k][j] = m.coef[k][has[k][j] ? e : lo[k]];
      }
    Fe<P> v[3][2], d[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        v[k][j] = fe_load<P>(z2 + (size_t)(has[k][j] ? cc[k][j] : 0u) * 32);
        d[k][j] = fe_load<P>(dict + (size_t)(has[k][j] ? kk[k][j] : 0u) * 32);
      }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (!has[k][j]) continue;
        const Fe<P> term = kk[k][j] == 0 ? v[k][j] : (kk[k][j] == 1 ? fe_neg(v[k][j]) : fe_mul(v[k][j], d[k][j]));
        acc[k] = fe_add(acc[k], term);
      }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = fe_group_sum<P, 64>(acc[k]);
  if (lane != 0) return;
  cross_finish<P>(az2, bz2, cz2, T, r, a1, b1, c1, fe_from_val<P>(u1), acc[0], acc[1], acc[2]);
}

// The cross term over the rows of the built-in MinRoot step circuits WITHOUT the sparse matrices: the 3t + 1 constraints
// InverseMinRootCircuit::synthesize records (src/nova/proof.rs:107-133, :219-227) are a fixed stencil over the round's own
// variables, so A z2, B z2, C z2 of a row are copies of witness values (and one four-term sum): no row pointers, no
// column / coefficient loads, no dependent gathers.  With S = seg_begin (first round variable), the step circuit's input
// z_in = (x, y, i) in the three variables before S, `one` the constant's column, PER = 4 (the reference's rounds: new_x,
// tmp1, tmp2, new_y) or 3 (bound form: tmp1, tmp2, new_y), round j and y_j = new_y_(j-1) (y_0 = z_in.y):
//   row 3j     x_j * x_j   = tmp1_j             x_j = new_x_(j-1)  (PER = 4; x_0 = z_in.x)
//   row 3j + 1 tmp1 * tmp1 = tmp2                   = y_(j-1) - i + j * one  (PER = 3, j > 0)
//   row 3j + 2 tmp2 * x_j  = new_y_j + y_j - i + (j + 1) * one
//   row 3t     final_i * one = i - t * one
// One row per lane (every running / fresh vector is read and written as contiguous 32-byte elements, like k_fold_many);
// the witness values a row needs sit in the 128 (96) bytes of its round and the one before.  Exact for ANY z2: the
// constant's coefficient is multiplied by z2[one] (1 in a fresh instance).  The host checks the stencil against the
// shape's triples before it uses this kernel (libvdf_nova.so public_params); other circuits keep k_nifs_cross.
// A z2, B z2, C z2 of stencil row i (0 .. 3t) from the witness: the part both stencil kernels share
template <class P, int PER>
__device__ __forceinline__ void minroot_stencil_row(const char* __restrict__ z2, size_t S, size_t one_col, uint64_t t, uint64_t i,
                                                    Fe<P>& a2, Fe<P>& b2, Fe<P>& c2) {
  const Fe<P> onev = fe_load<P>(z2 + one_col * 32);
  const Fe<P> i_in = fe_load<P>(z2 + (S - 1) * 32);
  // k * z2[one]: the constant's value is ONE in every fresh instance, and then the small-integer conversion is all it takes --
  // no Montgomery product (cross.cuh times_one; fe.cuh fe_from_small: ~50 instructions)
  const bool unit = fe_eq(onev, fe_one<P>());
  // The three kinds of row differ in WHERE their values sit, not in what is done with them: the addresses are selected
  // first and every load of the row is issued before the first use (a wavefront holds all three kinds: as branches they
  // would be three serial rounds of loads).  pa / pb / pc = the sources of A z2, B z2 and the first term of C z2.
  const bool last = i == 3 * t;
  const uint64_t j = last ? t - 1 : i / 3;
  const uint32_t role = last ? 3u : (uint32_t)(i - 3 * j);
  const char* rd = z2 + (S + (size_t)PER * j) * 32;                // this round's variables
  const char* t1p = rd + (PER - 3) * 32;                            // tmp1, tmp2, new_y
  const char* yp = j ? rd - 32 : z2 + (S - 2) * 32;                 // y_j = new_y_(j-1): the element right before this round
  // x_j: a variable (PER = 4: new_x_(j-1), or z_in.x), or y_(j-1) - i + j * one (PER = 3, j > 0; y_(-1) does not exist)
  const char* px = PER == 4 ? (j ? rd - (size_t)PER * 32 : z2 + (S - 3) * 32)
                            : (j == 0 ? z2 + (S - 3) * 32 : (j > 1 ? rd - (size_t)PER * 32 - 32 : z2 + (S - 2) * 32));
  const char* pa = role == 0 ? px : (role == 1 ? t1p : (role == 2 ? t1p + 32 : z2 + (S + (size_t)PER * t) * 32));
  const char* pb = role == 1 ? t1p : (role == 3 ? z2 + one_col * 32 : px);
  const char* pc = role == 3 ? z2 + (S - 1) * 32 : t1p + role * 32;
  a2 = fe_load<P>(pa); b2 = fe_load<P>(pb); c2 = fe_load<P>(pc);
  const Fe<P> y = fe_load<P>(yp);
  if (PER == 3 && j > 0) {                                          // the loaded value is y_(j-1): turn it into x_j
    const Fe<P> xa = fe_add(fe_sub(role == 0 ? a2 : b2, i_in), times_one(j, unit, onev));
    if (role == 0) { a2 = xa; b2 = xa; } else if (role == 2) b2 = xa;
  }
  if (role == 2) c2 = fe_add(fe_sub(fe_add(c2, y), i_in), times_one(j + 1, unit, onev));
  if (role == 3) c2 = fe_sub(c2, times_one(t, unit, onev));
}

template <class P, int PER>
__global__ __launch_bounds__(256) void k_nifs_cross_minroot(const char* __restrict__ z2, size_t S, size_t one_col, uint64_t t,
                                                            size_t row0, const char* __restrict__ az1, const char* __restrict__ bz1,
                                                            const char* __restrict__ cz1, FeVal u1, char* __restrict__ az2,
                                                            char* __restrict__ bz2, char* __restrict__ cz2, char* __restrict__ T) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > 3 * t) return;
  const size_t r = row0 + i;
  const Fe<P> a1 = fe_load<P>(az1 + r * 32), b1 = fe_load<P>(bz1 + r * 32), c1 = fe_load<P>(cz1 + r * 32);
  Fe<P> a2, b2, c2;
  minroot_stencil_row<P, PER>(z2, S, one_col, t, i, a2, b2, c2);
  cross_finish<P>(az2, bz2, cz2, T, r, a1, b1, c1, fe_from_val<P>(u1), a2, b2, c2);
}

// The same for the FORWARD step circuit over L lanes in one launch (VDF_CIRCUIT_MINROOT_FORWARD: L = 1, and _LANES).  Lane
// l = blockIdx.y owns the variables S = S0 + l (3t + 1) .. and the rows row0 + l (3t + 1) .., and ITS z_in = (x_0, y_0, i) sits at
// Z .. Z + 2, Z = S0 - 3L + 3l.  Round j holds x' = x_(j+1), tmp1, tmp2 at S + 3j .. S + 3j + 2 and final_i sits at S + 3t;
// x_0 = z_in.x, y_0 = z_in.y, and for j >= 1 y_j is no variable but x_(j-1) + i + (j - 1) * one:
//   row 3j     x' * x'     = tmp1
//   row 3j + 1 tmp1 * tmp1 = tmp2
//   row 3j + 2 tmp2 * x'   = x_j + y_j      (j = 0: z_in.x + z_in.y; j >= 1: x_j + x_(j-1) + i + (j - 1) * one)
//   row 3t     final_i * one = i + t * one
// Built like the inverse stencil: one row per lane, every source address selected first (columns, not pointers: a column that
// does not exist for a small j, rd - 6 below, is then never formed as an address; a lane's j < 2 rows read its own inputs, never
// the lane before), every load issued before the first use, the constant's coefficient times z2[one].  pd = the second term of
// C z2 of a role-2 row (a valid address in every lane, used by that role only).
template <class P>
__global__ __launch_bounds__(256) void k_nifs_cross_minroot_forward_lanes(const char* __restrict__ z2, size_t S0, uint32_t lanes, size_t one_col,
                                                                          uint64_t t, size_t row0, const char* __restrict__ az1,
                                                                          const char* __restrict__ bz1, const char* __restrict__ cz1, FeVal u1,
                                                                          char* __restrict__ az2, char* __restrict__ bz2, char* __restrict__ cz2,
                                                                          char* __restrict__ T) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const uint32_t lane = blockIdx.y;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > 3 * t) return;
  const size_t per_lane = 3 * (size_t)t + 1;
  const size_t S = S0 + (size_t)lane * per_lane;                     // this lane's first round variable
  const size_t Z = S0 - (size_t)3 * lanes + (size_t)3 * lane;        // this lane's z_in.x
  const size_t r = row0 + (size_t)lane * per_lane + i;
  const bool last = i == 3 * t;
  const uint64_t j = last ? t - 1 : i / 3;
  const uint32_t role = last ? 3u : (uint32_t)(i - 3 * j);
  const size_t rd = S + (size_t)3 * j;                               // this round's x', tmp1, tmp2
  const size_t cxj = j ? rd - 3 : Z;                                 // x_j
  const size_t ca = role == 3 ? S + (size_t)3 * t : rd + role;
  const size_t cb = role == 1 ? rd + 1 : (role == 3 ? one_col : rd);
  const size_t cc = role == 2 ? cxj : (role == 3 ? Z + 2 : rd + role + 1);
  const size_t cd = j >= 2 ? rd - 6 : (j == 1 ? Z : Z + 1);          // j >= 2: x_(j-1); j = 1: x_0 = z_in.x; j = 0: y_0 = z_in.y
  const char *pa = z2 + ca * 32, *pb = z2 + cb * 32, *pc = z2 + cc * 32, *pd = z2 + cd * 32;
  const Fe<P> a1 = fe_load<P>(az1 + r * 32), b1 = fe_load<P>(bz1 + r * 32), c1 = fe_load<P>(cz1 + r * 32);
  const Fe<P> onev = fe_load<P>(z2 + one_col * 32);
  const Fe<P> i_in = fe_load<P>(z2 + (Z + 2) * 32);
  const Fe<P> a2 = fe_load<P>(pa), b2 = fe_load<P>(pb);
  Fe<P> c2 = fe_load<P>(pc);
  const Fe<P> d = fe_load<P>(pd);
  const bool unit = fe_eq(onev, fe_one<P>());                        // ONE in every fresh instance: a uniform branch
  if (role == 2) {
    c2 = fe_add(c2, d);
    if (j > 0) c2 = fe_add(fe_add(c2, i_in), times_one(j - 1, unit, onev));
  }
  if (role == 3) c2 = fe_add(c2, times_one(t, unit, onev));
  cross_finish<P>(az2, bz2, cz2, T, r, a1, b1, c1, fe_from_val<P>(u1), a2, b2, c2);
}

// y * r for a scalar r below 2^128 given as a PLAIN integer (four limbs), y and the result in Montgomery form: the fold
// challenges of NIFS are 128-bit (CHAL_BITS), so  y R * r  is a 383-bit integer whose residue is the Montgomery form of y r
// -- no Montgomery reduction at all.  With m = 2^254 + c (c = the low four limbs of the modulus, below 2^126):
//   P = y r = Ph 2^254 + Pl,  Pl < 2^254,  Ph <= 2^128   (y < m, r < 2^128),   P = Pl - c Ph  (mod m),   c Ph < 2^254 < m:
// both terms are canonical, one fe_sub finishes.  32 + 16 limb products instead of the 96 of a Montgomery multiplication.
template <class P>
__device__ __forceinline__ Fe<P> fe_mul_u128(const Fe<P>& y, const uint32_t r[4]) {
  uint32_t p[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) p[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t t = (uint64_t)y.v[j] * r[i] + p[i + j] + carry;        // <= 2^64 - 1: no overflow
      p[i + j] = (uint32_t)t;
      carry = (uint32_t)(t >> 32);
    }
    p[i + 8] = carry;
  }
  uint32_t ph[5];
#pragma unroll
  for (int k = 0; k < 4; ++k) ph[k] = (p[7 + k] >> 30) | (p[8 + k] << 2);
  ph[4] = p[11] >> 30;                                                       // 0 or 1 (Ph <= 2^128)
  Fe<P> lo;
#pragma unroll
  for (int i = 0; i < 7; ++i) lo.v[i] = p[i];
  lo.v[7] = p[7] & 0x3FFFFFFFu;
  uint32_t d[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) d[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                              // c = MOD[0..3]
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const uint64_t t = (uint64_t)ph[j] * P::MOD[i] + d[i + j] + carry;
      d[i + j] = (uint32_t)t;
      carry = (uint32_t)(t >> 32);
    }
    d[i + 5] = carry;
  }
  Fe<P> hi;
#pragma unroll
  for (int i = 0; i < 8; ++i) hi.v[i] = d[i];                               // (d[8] = 0: c Ph < 2^254)
  return fe_sub(lo, hi);
}

// The stencil rows WITH the previous step's fold of those rows applied on the way: the rows' cross term needs
// the running A z, B z, C z folded with the previous fresh ones -- which this very kernel wrote a step ago into az2 / bz2 / cz2
// and is about to overwrite.  So each lane reads its row of the running vectors AND of the previous fresh ones, folds
// (X1 <- X1 + r X2prev; E1 <- E1 + r Tprev when e1 is given), stores the folded row, and goes on as k_nifs_cross_minroot does
// with the folded values.  One pass over the row's 7 (8) streams instead of a 5-vector k_fold_many over ALL rows in front of
// it on the step's longest dependent path; the fold of z and of the ~10^4 other rows runs elsewhere, off that path.
// U128: r is a plain integer below 2^128 (every NIFS challenge: fe_mul_u128, no Montgomery reduction), else Montgomery form.
template <class P, int PER, bool U128>
__global__ __launch_bounds__(256) void k_nifs_cross_minroot_fold(const char* __restrict__ z2, size_t S, size_t one_col, uint64_t t,
                                                                 size_t row0, FeVal rv, char* __restrict__ az1, char* __restrict__ bz1,
                                                                 char* __restrict__ cz1, char* __restrict__ e1, const char* tprev,
                                                                 FeVal u1, char* az2, char* bz2, char* cz2, char* T) {
  __builtin_amdgcn_s_setprio(3);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > 3 * t) return;
  const size_t r = row0 + i;
  Fe<P> a1 = fe_load<P>(az1 + r * 32), b1 = fe_load<P>(bz1 + r * 32), c1 = fe_load<P>(cz1 + r * 32);
  const Fe<P> ap = fe_load<P>(az2 + r * 32), bp = fe_load<P>(bz2 + r * 32), cp = fe_load<P>(cz2 + r * 32);
  Fe<P> a2, b2, c2;
  minroot_stencil_row<P, PER>(z2, S, one_col, t, i, a2, b2, c2);
  const uint32_t rr[4] = {rv.v[0], rv.v[1], rv.v[2], rv.v[3]};
  const Fe<P> rm = fe_from_val<P>(rv);
  auto times_r = [&](const Fe<P>& y) -> Fe<P> { return U128 ? fe_mul_u128<P>(y, rr) : fe_mul(rm, y); };
  if (e1) {
    const Fe<P> e = fe_load<P>(e1 + r * 32), tp = fe_load<P>(tprev + r * 32);
    fe_store<P>(e1 + r * 32, fe_add(e, times_r(tp)));
  }
  a1 = fe_add(a1, times_r(ap));
  b1 = fe_add(b1, times_r(bp));
  c1 = fe_add(c1, times_r(cp));
  fe_store<P>(az1 + r * 32, a1);
  fe_store<P>(bz1 + r * 32, b1);
  fe_store<P>(cz1 + r * 32, c1);
  cross_finish<P>(az2, bz2, cz2, T, r, a1, b1, c1, fe_from_val<P>(u1), a2, b2, c2);
}

// acc_k <- acc_k + r * add_k for up to 8 vectors in one launch (the witness fold W, E and the running Az, Bz, Cz)
struct FoldArgs { char* acc[8]; const char* add[8]; uint32_t blk_end[8]; uint64_t n[8]; int k; };
template <class P>
__global__ __launch_bounds__(256) void k_fold_many(FoldArgs a, FeVal rv) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  int seg = 0;
  while (seg < a.k - 1 && blockIdx.x >= a.blk_end[seg]) ++seg;
  const uint32_t blk0 = seg ? a.blk_end[seg - 1] : 0u;
  const size_t i = (size_t)(blockIdx.x - blk0) * 256 + threadIdx.x;
  if (i >= a.n[seg]) return;
  const Fe<P> r = fe_from_val<P>(rv);
  const Fe<P> x = fe_load<P>(a.acc[seg] + i * 32);
  const Fe<P> y = fe_load<P>(a.add[seg] + i * 32);
  fe_store<P>(a.acc[seg] + i * 32, fe_add(x, fe_mul(r, y)));
}
// the same with r below 2^128, as a plain integer in rv.v[0..3] (every fold challenge: fe_mul_u128)
template <class P>
__global__ __launch_bounds__(256) void k_fold_many_u128(FoldArgs a, FeVal rv) {
  __builtin_amdgcn_s_setprio(3);
  int seg = 0;
  while (seg < a.k - 1 && blockIdx.x >= a.blk_end[seg]) ++seg;
  const uint32_t blk0 = seg ? a.blk_end[seg - 1] : 0u;
  const size_t i = (size_t)(blockIdx.x - blk0) * 256 + threadIdx.x;
  if (i >= a.n[seg]) return;
  const uint32_t r[4] = {rv.v[0], rv.v[1], rv.v[2], rv.v[3]};
  const Fe<P> x = fe_load<P>(a.acc[seg] + i * 32);
  const Fe<P> y = fe_load<P>(a.add[seg] + i * 32);
  fe_store<P>(a.acc[seg] + i * 32, fe_add(x, fe_mul_u128<P>(y, r)));
}

template <class P>
__global__ __launch_bounds__(256) void k_mul(const char* __restrict__ a, const char* __restrict__ b, size_t n,
                                             char* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fe_store<P>(out + i * 32, fe_mul(fe_load<P>(a + i * 32), fe_load<P>(b + i * 32)));
}

template <class P, int DIR>
__global__ __launch_bounds__(256) void k_mont(const char* __restrict__ a, size_t n, char* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fe<P> x = fe_load<P>(a + i * 32);
  fe_store<P>(out + i * 32, DIR ? fe_to_mont(x) : fe_from_mont(x));
}

template <class P>
__global__ __launch_bounds__(256) void k_mul_chain(const char* __restrict__ a, size_t n, int iters,
                                                   char* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fe<P> x = fe_load<P>(a + i * 32);
  Fe<P> y = x;
  for (int k = 0; k < iters; ++k) y = fe_mul(y, x);
  fe_store<P>(out + i * 32, y);
}

// Box fingerprint (bench.py): every SIMD runs `iters` dependent Montgomery products; s_memtime counts shader clocks,
// s_memrealtime the constant 100 MHz reference, so their ratio over all wavefronts is the clock the device sustained
// under the integer load the MSM puts on it.  out[0] += shader cycles, out[1] += reference ticks (one add per wavefront).
__global__ __launch_bounds__(256) void k_clock_probe(int iters, unsigned long long* __restrict__ out) {
  Fe<FpParams> x, y;
#pragma unroll
  for (int i = 0; i < 8; ++i) { x.v[i] = threadIdx.x * 2654435761u + i; y.v[i] = blockIdx.x * 40503u + i * 7 + 1; }
  x.v[7] &= 0x3fffffffu; y.v[7] &= 0x3fffffffu;
  const uint64_t c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int k = 0; k < iters; ++k) y = fe_mul_lazy(y, x);
  const uint64_t c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out, (unsigned long long)(c1 - c0));
    atomicAdd(out + 1, (unsigned long long)(r1 - r0));
  }
  if (y.v[0] == 0x12345678u && y.v[5] == 0x9abcdef0u) out[2] = y.v[1];          // keeps the chain alive
}

Status vec_axpy(int field, const void* a, const void* r, const void* b, size_t n, void* out, hipStream_t s) {
  if (n == 0) return Status{};
  KTimer kt(s, "k_axpy", 96.0 * n);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_axpy<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, cbytes_of(a), cbytes_of(r), cbytes_of(b), n, bytes_of(out));
  });
}

Status vec_cross_term(int field, const void* az1, const void* bz1, const void* cz1, const void* az2, const void* bz2,
                      const void* cz2, const void* u1, size_t n, void* T, hipStream_t s) {
  if (n == 0) return Status{};
  KTimer kt(s, "k_cross_term", 224.0 * n);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_cross_term<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, cbytes_of(az1), cbytes_of(bz1), cbytes_of(cz1), cbytes_of(az2),
                       cbytes_of(bz2), cbytes_of(cz2), cbytes_of(u1), n, bytes_of(T));
  });
}

Status vec_minroot_witness(int field, const void* trace_xy, const void* i0, uint64_t t, void* W, hipStream_t s) {
  KTimer kt(s, "k_minroot_witness", 192.0 * t);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_minroot_witness<tag_t<decltype(f)>>), grid_for(t + 1), dim3(256), 0, s, cbytes_of(trace_xy), cbytes_of(i0), t, bytes_of(W));
  });
}

Status vec_spmv_long(int field, const uint32_t* const rowptr[3], const uint32_t* const col[3], const uint32_t* const coef[3],
                     const void* dict, const void* z, const uint32_t* long_rows, size_t n_long, void* const out[3], hipStream_t s) {
  if (n_long == 0) return Status{};
  Csr3 m;
  for (int k = 0; k < 3; ++k) { m.rowptr[k] = rowptr[k]; m.col[k] = col[k]; m.coef[k] = coef[k]; }
  KTimer kt(s, "k_spmv_long", 0.0);                    // priced with the cross term that reads its results
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_spmv_long<tag_t<decltype(f)>>), dim3((unsigned)((n_long + 3) / 4)), dim3(256), 0, s, m, cbytes_of(dict), cbytes_of(z), long_rows,
                       n_long, bytes_of(out[0]), bytes_of(out[1]), bytes_of(out[2]));
  });
}

Status vec_spmv(int field, const uint32_t* rowptr, const uint32_t* col, const uint32_t* coef, const void* dict,
                const void* z, size_t rows, void* out, hipStream_t s) {
  if (rows == 0) return Status{};
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_spmv<tag_t<decltype(f)>>), grid_for(rows), dim3(256), 0, s, rowptr, col, coef, cbytes_of(dict), cbytes_of(z), rows, bytes_of(out));
  });
}

static FeVal to_val(const vdf_fe* p) { FeVal v; std::memcpy(v.v, p, 32); return v; }

Status vec_step_z(int field, const void* trace_xy, uint64_t t, const vdf_fe z_in[3], const vdf_fe* i0, const vdf_fe* u,
                  const vdf_fe X[6], void* z, void* packed, hipStream_t s) {
  StepConsts k;
  for (int i = 0; i < 3; ++i) k.z_in[i] = to_val(&z_in[i]);
  k.i0 = to_val(i0);
  k.u = to_val(u);
  for (int i = 0; i < 6; ++i) k.X[i] = to_val(&X[i]);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_step_z<tag_t<decltype(f)>>), grid_for(t + 1), dim3(256), 0, s, cbytes_of(trace_xy), k, t, bytes_of(z), bytes_of(packed));
  });
}

Status vec_step_segment(int field, const void* trace_xy, uint64_t t, const vdf_fe* i0, int per, void* out, void* packed,
                        const vdf_fe* i_in, hipStream_t s) {
  KTimer kt(s, "k_step_segment", (64.0 + 32.0 * per) * t);    // trace (x, y) read + `per` variables written per round
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_step_segment<tag_t<decltype(f)>>), grid_for(t + 1), dim3(256), 0, s, cbytes_of(trace_xy), to_val(i0), t, per, bytes_of(out),
                       bytes_of(packed), to_val(i_in ? i_in : i0));
  });
}

Status vec_forward_segment_lanes(int field, const void* trace_xy, size_t lane_stride, uint64_t t, size_t lanes, const vdf_fe* i_end, void* out,
                                 hipStream_t s) {
  if (lanes == 0 || lanes > VDF_MINROOT_MAX_LANES || lane_stride < t + 1) return Status{VDF_ERR_BAD_ARG, "bad lanes"};
  LaneEnds e;
  std::memset(&e, 0, sizeof(e));
  for (size_t l = 0; l < lanes; ++l) e.v[l] = to_val(&i_end[l]);
  // trace x read + three variables written per round; a single chain keeps the label it always had
  KTimer kt(s, lanes == 1 ? "k_forward_segment" : "k_forward_segment_lanes", (32.0 + 96.0) * t * lanes);
  const dim3 grid(grid_for(t + 1).x, (unsigned)lanes);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_forward_segment_lanes<tag_t<decltype(f)>>), grid, dim3(256), 0, s, cbytes_of(trace_xy), lane_stride, e, t, bytes_of(out));
  });
}

// lanes per row: 8 for the ~10^4 rows a step waits for (latency), 4 for long runs of short rows (the MinRoot rounds: all
// gathers of a row at once), 1 = the lane-per-row kernel.  vdf_hip_tuning.nifs_lanes = 1 | 4 | 8 forces one (tuning / A-B measurements).
int nifs_cross_lanes(size_t rows) {
  const int forced = tuning().nifs_lanes;
  return forced == 1 || forced == 4 || forced == 8 ? forced : (rows <= (1u << 15) ? 8 : 1);
}

// With `long_rowlist` (the distinct rows that have a matrix of more than VDF_LONG_ROW entries) the launch sums those rows
// itself (k_nifs_cross_f; the caller checked nifs_cross_lanes(rows) == 8); without, vec_spmv_long ran before it.
Status vec_nifs_cross(int field, const uint32_t* const rowptr[3], const uint32_t* const col[3],
                      const uint32_t* const coef[3], const void* dict, const CrossOperands& o, size_t rows, size_t skip_begin,
                      size_t skip_len, const uint32_t* long_rowlist, size_t n_long_rows, double alg_bytes, hipStream_t s) {
  if (rows == 0) return Status{};
  Csr3 m;
  for (int k = 0; k < 3; ++k) { m.rowptr[k] = rowptr[k]; m.col[k] = col[k]; m.coef[k] = coef[k]; }
  const int lpr = nifs_cross_lanes(rows);
  if (long_rowlist && n_long_rows) {
    if (lpr != 8) return Status{VDF_ERR_BAD_ARG, "the fused cross term runs eight lanes per row"};
    KTimer kt(s, "k_nifs_cross_f", alg_bytes);
    const uint32_t long_wgs = (uint32_t)((n_long_rows + 3) / 4);
    const dim3 grid((unsigned)((rows + 31) / 32) + long_wgs);
    return with_field(field, [&](auto f) {
      hipLaunchKernelGGL((k_nifs_cross_f<tag_t<decltype(f)>>), grid, dim3(256), 0, s, m, cbytes_of(dict), cbytes_of(o.z2), cbytes_of(o.abc1[0]),
                         cbytes_of(o.abc1[1]), cbytes_of(o.abc1[2]), to_val(o.u1), rows, skip_begin, skip_len, long_rowlist, n_long_rows, long_wgs,
                         bytes_of(o.abc2[0]), bytes_of(o.abc2[1]), bytes_of(o.abc2[2]), bytes_of(o.T));
    });
  }
  KTimer kt(s, lpr == 1 ? "k_nifs_cross" : (lpr == 4 ? "k_nifs_cross_w4" : "k_nifs_cross_w8"), alg_bytes);
  if (lpr == 1)
    return with_field(field, [&](auto f) {
      hipLaunchKernelGGL((k_nifs_cross<tag_t<decltype(f)>>), grid_for(rows), dim3(256), 0, s, m, cbytes_of(dict), cbytes_of(o.z2), cbytes_of(o.abc1[0]),
                         cbytes_of(o.abc1[1]), cbytes_of(o.abc1[2]), to_val(o.u1), rows, skip_begin, skip_len, bytes_of(o.abc2[0]), bytes_of(o.abc2[1]),
                         bytes_of(o.abc2[2]), bytes_of(o.T));
    });
  const dim3 grid((unsigned)((rows + 256 / lpr - 1) / (256 / lpr)));       // 64 rows of 4 lanes or 32 rows of 8 per workgroup
  return with_int<4, 8>(lpr, "lanes per row", [&](auto lanes) {
    return with_field(field, [&](auto f) {
      hipLaunchKernelGGL((k_nifs_cross_w<tag_t<decltype(f)>, lanes.value>), grid, dim3(256), 0, s, m, cbytes_of(dict), cbytes_of(o.z2), cbytes_of(o.abc1[0]),
                         cbytes_of(o.abc1[1]), cbytes_of(o.abc1[2]), to_val(o.u1), rows, skip_begin, skip_len, bytes_of(o.abc2[0]), bytes_of(o.abc2[1]),
                         bytes_of(o.abc2[2]), bytes_of(o.T));
    });
  });
}

static constexpr const char* BAD_PER = "variables per round must be 3 or 4";
Status vec_nifs_cross_minroot(int field, int per, uint64_t t, size_t seg_begin, size_t one_col, size_t row0, const CrossOperands& o,
                              hipStream_t s) {
  if (per != 3 && per != 4) return Status{VDF_ERR_BAD_ARG, BAD_PER};
  if (t == 0 || seg_begin < 3) return Status{VDF_ERR_BAD_ARG, "bad segment"};
  const size_t rows = 3 * (size_t)t + 1;
  // algorithmic bytes: 3 running + 3 fresh + T elements per row, and the round's variables once (SURVEY 8d counts 224 B per
  // row for the cross term alone and the sparse products apart; here the products are the witness copies themselves)
  KTimer kt(s, "k_nifs_cross_minroot", (double)rows * 7 * 32 + (double)per * t * 32);
  const dim3 grid = grid_for(rows);
  return with_field(field, [&](auto f) {
    return with_int<4, 3>(per, BAD_PER, [&](auto perv) {
      hipLaunchKernelGGL((k_nifs_cross_minroot<tag_t<decltype(f)>, perv.value>), grid, dim3(256), 0, s, cbytes_of(o.z2), seg_begin, one_col, t, row0,
                         cbytes_of(o.abc1[0]), cbytes_of(o.abc1[1]), cbytes_of(o.abc1[2]), to_val(o.u1), bytes_of(o.abc2[0]), bytes_of(o.abc2[1]),
                         bytes_of(o.abc2[2]), bytes_of(o.T));
    });
  });
}

Status vec_nifs_cross_minroot_forward_lanes(int field, uint64_t t, size_t lanes, size_t seg_begin, size_t one_col, size_t row0,
                                            const CrossOperands& o, hipStream_t s) {
  if (t == 0 || lanes == 0 || lanes > VDF_MINROOT_MAX_LANES || seg_begin < 3 * lanes) return Status{VDF_ERR_BAD_ARG, "bad segment"};
  const size_t rows = 3 * (size_t)t + 1;
  // priced as the inverse stencil is; the labels are short on purpose (a timed launch keeps 23 characters, and the fused inverse
  // stencil's begins the same way), and a single chain keeps the one it always had
  KTimer kt(s, lanes == 1 ? "k_nifs_cross_fwd" : "k_nifs_cross_fwd_lanes", ((double)rows * 7 * 32 + 3.0 * t * 32) * lanes);
  const dim3 grid(grid_for(rows).x, (unsigned)lanes);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_nifs_cross_minroot_forward_lanes<tag_t<decltype(f)>>), grid, dim3(256), 0, s, cbytes_of(o.z2), seg_begin, (uint32_t)lanes,
                       one_col, t, row0, cbytes_of(o.abc1[0]), cbytes_of(o.abc1[1]), cbytes_of(o.abc1[2]), to_val(o.u1), bytes_of(o.abc2[0]),
                       bytes_of(o.abc2[1]), bytes_of(o.abc2[2]), bytes_of(o.T));
  });
}

// r: Montgomery form (host); sent as a plain integer when it is below 2^128 and tuning().fold_u128 allows (as vec_fold_many does)
template <class P> static bool plain_if_u128(const vdf_fe* r, FeVal& out) {
  Fe<P> t; memcpy(t.v, r, 32); t = fe_from_mont(t); memcpy(out.v, t.v, 32);
  return (out.v[4] | out.v[5] | out.v[6] | out.v[7]) == 0;
}
Status vec_nifs_cross_minroot_fold(int field, int per, uint64_t t, size_t seg_begin, size_t one_col, size_t row0, const vdf_fe* r,
                                   void* const folded[3], void* e1, const void* tprev, const CrossOperands& o, hipStream_t s) {
  if (per != 3 && per != 4) return Status{VDF_ERR_BAD_ARG, BAD_PER};
  if (t == 0 || seg_begin < 3) return Status{VDF_ERR_BAD_ARG, "bad segment"};
  const size_t rows = 3 * (size_t)t + 1;
  // algorithmic bytes: the row of 3 running vectors read and written, 3 previous fresh read, 3 fresh + T written (E and the
  // previous T: read, read, written), and the round's variables once
  KTimer kt(s, "k_nifs_cross_minroot_fold", (double)rows * (13 + (e1 ? 3 : 0)) * 32 + (double)per * t * 32);
  const dim3 grid = grid_for(rows);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    FeVal plain{};
    const bool small = tuning().fold_u128 && plain_if_u128<P>(r, plain);
    const FeVal rv = small ? plain : to_val(r);
    return with_int<4, 3>(per, BAD_PER, [&](auto perv) {
      return with_bool(small, [&](auto u128) {
        hipLaunchKernelGGL((k_nifs_cross_minroot_fold<P, perv.value, u128.value>), grid, dim3(256), 0, s, cbytes_of(o.z2), seg_begin, one_col, t, row0,
                           rv, bytes_of(folded[0]), bytes_of(folded[1]), bytes_of(folded[2]), bytes_of(e1), cbytes_of(tprev), to_val(o.u1),
                           bytes_of(o.abc2[0]), bytes_of(o.abc2[1]), bytes_of(o.abc2[2]), bytes_of(o.T));
      });
    });
  });
}

Status vec_fold_many(int field, const vdf_fe* r, int k, void* const acc[], const void* const add[], const size_t n[],
                     hipStream_t s) {
  if (k <= 0) return Status{};
  if (k > 8) return Status{VDF_ERR_BAD_ARG, "at most 8 vectors per fold"};
  FoldArgs a{};
  a.k = k;
  uint64_t blocks = 0;
  for (int i = 0; i < k; ++i) {
    a.acc[i] = bytes_of(acc[i]); a.add[i] = cbytes_of(add[i]); a.n[i] = n[i];
    blocks += (n[i] + 255) / 256;
    if (blocks >= (1ull << 31)) return Status{VDF_ERR_BAD_LENGTH, "fold too large"};
    a.blk_end[i] = (uint32_t)blocks;
  }
  if (blocks == 0) return Status{};
  double elems = 0;
  for (int i = 0; i < k; ++i) elems += (double)n[i];
  KTimer kt(s, "k_fold_many", 96.0 * elems);
  // a challenge below 2^128 (every NIFS fold): its plain value travels instead, and the product needs no Montgomery reduction
  FeVal plain{};
  bool small = false;
  if (tuning().fold_u128) VDF_TRY(with_field(field, [&](auto f) { small = plain_if_u128<tag_t<decltype(f)>>(r, plain); return Status{}; }));
  if (small)
    return with_field(field, [&](auto f) {
      hipLaunchKernelGGL((k_fold_many_u128<tag_t<decltype(f)>>), dim3((unsigned)blocks), dim3(256), 0, s, a, plain);
    });
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_fold_many<tag_t<decltype(f)>>), dim3((unsigned)blocks), dim3(256), 0, s, a, to_val(r));
  });
}

// ---- random linear combinations of many instances (vdf_nova_verify_batch) -------------------------------------------
// out[i] = sum_j w[j] v[j][i], v[j][i] = 0 for i >= n[j]; w[j] a plain integer below 2^128 (fe_mul_u128, as k_fold_many_u128).
// One pass: every lane reads its element of each vector once and writes its output once, the sum in registers.  `out` may
// be one of the vectors (a lane reads all of its inputs before it stores).
struct LincombArgs { const char* v[LINCOMB_MAX]; uint64_t n[LINCOMB_MAX]; uint32_t w[LINCOMB_MAX][4]; int count; };
template <class P>
__global__ __launch_bounds__(256) void k_lincomb_u128(LincombArgs a, size_t n_out, char* out) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_out) return;
  Fe<P> acc = fe_zero<P>();
  // four vectors' loads in flight before their products
  for (int j = 0; j < a.count; j += 4) {
    Fe<P> x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = j + k < a.count && i < a.n[j + k] ? fe_load<P>(a.v[j + k] + i * 32) : fe_zero<P>();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (j + k >= a.count) break;
      const uint32_t r[4] = {a.w[j + k][0], a.w[j + k][1], a.w[j + k][2], a.w[j + k][3]};
      acc = fe_add(acc, fe_mul_u128<P>(x[k], r));
    }
  }
  fe_store<P>(out + i * 32, acc);
}

// out[r] = sum_q rho_q ((A z_q)[r] (B z_q)[r] - u_q (C z_q)[r] - E_q[r]): the relaxed R1CS residuals of many instances of one
// shape, randomly combined, in one pass over the rows.  The instances are an argument block in device memory (uniform loads).
// The first `long_wgs` workgroups give each row that has a matrix of more than VDF_LONG_ROW entries one wavefront (as
// k_spmv_long: lanes stride over the entries, then a butterfly sum); the rest take one short row per lane, with the row's
// first entries (column, coefficient index, dictionary value) loaded once in k_nifs_cross's three waves and the instances
// looped over inside the lane.
struct ResidualItem { const char* z; const char* E; uint32_t u[8]; uint32_t rho[4]; };
static_assert(sizeof(ResidualItem) == 64, "argument block layout");
template <class P>
__device__ __forceinline__ Fe<P> residual_term(const Fe<P>& a, const Fe<P>& b, const Fe<P>& c, const ResidualItem& it, size_t r) {
  Fe<P> u;
#pragma unroll
  for (int k = 0; k < 8; ++k) u.v[k] = it.u[k];
  Fe<P> t = fe_sub(fe_mul(a, b), fe_mul(u, c));
  if (it.E) t = fe_sub(t, fe_load<P>(it.E + r * 32));
  const uint32_t rho[4] = {it.rho[0], it.rho[1], it.rho[2], it.rho[3]};
  return fe_mul_u128<P>(t, rho);
}
template <class P>
__global__ __launch_bounds__(256) void k_relaxed_residual_batch(Csr3 m, const char* __restrict__ dict, const ResidualItem* __restrict__ items,
                                                                int count, size_t rows, const uint32_t* __restrict__ long_rowlist,
                                                                size_t n_long, uint32_t long_wgs, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  if (blockIdx.x < long_wgs) {
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_long) return;                                        // whole wavefronts leave together
    const uint32_t lane = threadIdx.x & 63, r = long_rowlist[w];
    uint32_t lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = m.rowptr[k][r]; hi[k] = m.rowptr[k][r + 1]; }
    Fe<P> acc = fe_zero<P>();
    for (int q = 0; q < count; ++q) {
      const ResidualItem& it = items[q];
      Fe<P> s[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s[k] = fe_zero<P>();
        for (uint32_t e = lo[k] + lane; e < hi[k]; e += 64)
          s[k] = fe_add(s[k], spmv_term<P>(fe_load<P>(it.z + (size_t)m.col[k][e] * 32), m.coef[k][e], dict));
        s[k] = fe_group_sum<P, 64>(s[k]);
      }
      if (lane == 0) acc = fe_add(acc, residual_term<P>(s[0], s[1], s[2], it, r));
    }
    if (lane == 0) fe_store<P>(out + (size_t)r * 32, acc);
    return;
  }
  const size_t r = (size_t)(blockIdx.x - long_wgs) * 256 + threadIdx.x;
  if (r >= rows) return;
  uint32_t lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = m.rowptr[k][r]; hi[k] = m.rowptr[k][r + 1]; }
  if (hi[0] - lo[0] > VDF_LONG_ROW || hi[1] - lo[1] > VDF_LONG_ROW || hi[2] - lo[2] > VDF_LONG_ROW) return;   // a wavefront's row
  constexpr int PRE[3] = {2, 2, 4};
  uint32_t cc[3][4], kk[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < PRE[k]; ++j) {
      const uint32_t e = lo[k] + j < hi[k] ? lo[k] + j : lo[k];       // (arrays are nnz + 1 long: lo is always readable)
      cc[k][j] = lo[k] + j < hi[k] ? m.col[k][e] : 0u;
      kk[k][j] = lo[k] + j < hi[k] ? m.coef[k][e] : 0u;
    }
  Fe<P> dv[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < PRE[k]; ++j) dv[k][j] = kk[k][j] > 1 ? fe_load<P>(dict + (size_t)kk[k][j] * 32) : fe_zero<P>();
  Fe<P> acc = fe_zero<P>();
  for (int q = 0; q < count; ++q) {
    const ResidualItem& it = items[q];
    Fe<P> v[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < PRE[k]; ++j) v[k][j] = fe_load<P>(it.z + (size_t)cc[k][j] * 32);
    Fe<P> s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s[k] = fe_zero<P>();
#pragma unroll
      for (int j = 0; j < PRE[k]; ++j) {
        if (lo[k] + j >= hi[k]) break;
        const uint32_t ci = kk[k][j];
        s[k] = ci == 0 ? fe_add(s[k], v[k][j]) : ci == 1 ? fe_sub(s[k], v[k][j]) : fe_add(s[k], fe_mul(v[k][j], dv[k][j]));
      }
      for (uint32_t e = lo[k] + PRE[k]; e < hi[k]; ++e)
        s[k] = fe_add(s[k], spmv_term<P>(fe_load<P>(it.z + (size_t)m.col[k][e] * 32), m.coef[k][e], dict));
    }
    acc = fe_add(acc, residual_term<P>(s[0], s[1], s[2], it, r));
  }
  fe_store<P>(out + r * 32, acc);
}

Status vec_lincomb_u128(int field, int count, const void* const v[], const size_t n[], const vdf_fe w[], size_t n_out, void* out,
                        hipStream_t s) {
  if (n_out == 0) return Status{};
  if (count < 1 || count > LINCOMB_MAX) return Status{VDF_ERR_BAD_ARG, "1..64 vectors"};
  if ((n_out + 255) / 256 >= (1ull << 31)) return Status{VDF_ERR_BAD_LENGTH, "combination too long"};
  LincombArgs a{};
  a.count = count;
  double elems = (double)n_out;
  for (int j = 0; j < count; ++j) {
    a.v[j] = cbytes_of(v[j]); a.n[j] = n[j];
    memcpy(a.w[j], w[j].l, 16);
    elems += (double)n[j];
  }
  KTimer kt(s, "k_lincomb_u128", 32.0 * elems);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_lincomb_u128<tag_t<decltype(f)>>), grid_for(n_out), dim3(256), 0, s, a, n_out, bytes_of(out));
  });
}

Status vec_relaxed_residual_batch(int field, const uint32_t* const rowptr[3], const uint32_t* const col[3], const uint32_t* const coef[3],
                                  const void* dict, const void* block, int count, size_t rows, const uint32_t* long_rowlist,
                                  size_t n_long_rows, void* out, double alg_bytes, hipStream_t s) {
  if (rows == 0 || count == 0) return Status{};
  Csr3 m;
  for (int k = 0; k < 3; ++k) { m.rowptr[k] = rowptr[k]; m.col[k] = col[k]; m.coef[k] = coef[k]; }
  const uint32_t long_wgs = long_rowlist ? (uint32_t)((n_long_rows + 3) / 4) : 0u;
  KTimer kt(s, "k_relaxed_residual_batch", alg_bytes);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_relaxed_residual_batch<tag_t<decltype(f)>>), dim3((unsigned)((rows + 255) / 256) + long_wgs), dim3(256), 0, s, m, cbytes_of(dict),
                       reinterpret_cast<const ResidualItem*>(block), count, rows, long_rowlist, n_long_rows, long_wgs, bytes_of(out));
  });
}
void residual_pack(int count, const void* const z[], const void* const E[], const vdf_fe u[], const vdf_fe rho[], void* block) {
  ResidualItem* it = reinterpret_cast<ResidualItem*>(block);
  for (int q = 0; q < count; ++q) {
    it[q].z = cbytes_of(z[q]);
    it[q].E = E ? cbytes_of(E[q]) : nullptr;
    memcpy(it[q].u, u[q].l, 32);
    memcpy(it[q].rho, rho[q].l, 16);
  }
}
size_t residual_item_bytes() { return sizeof(ResidualItem); }

// ---- multi-point sparse evaluation (vdf_nova_verify_compressed_batch) ------------------------------------------------
// out[q] = sum over the entries (x, y, v) of A, B, C of  ex_q[x] w_q(matrix) v ey_q[ycol(y)],  w_q = 1, rho_q, rho_q^2:
// M(r_x, r_y) of many proofs in one pass over the rows, with no transposed product and no M vector.  Rows are taken as
// k_relaxed_residual_batch takes them (one lane per short row with its first PRE entries loaded once; the first `long_wgs`
// workgroups give every row of the long-row list one wavefront whose lanes stride the entries).  Per instance a lane forms
// ex_q[r] (s_A + rho_q s_B + rho_q^2 s_C) of ITS entries -- the term is linear in the entries, so a long row's lanes need no
// sum of their own: the workgroup's reduction adds them.  CH instances per pass keep their terms in registers; at the end of
// a pass: butterfly over the wave, LDS over the four waves, one partial per workgroup and instance (partials[q][workgroup]).
// Field addition is exact and commutative: no atomics, and the result does not depend on the order.
// ycol(y) = y below col_split, else col_hi_base + (y - col_split): the padded layout of the compression argument.
struct EvalItem { const char* ex; const char* ey; uint32_t rho[8]; uint32_t rho2[8]; };
static_assert(sizeof(EvalItem) == 80, "argument block layout");
// instances per pass, by the register report: 2 = 244 VGPRs, two waves per SIMD; 4 = 256 + 5 AGPRs, one wave; 8 goes
// to scratch memory.  `make ab AB_FLAGS=-DVDF_SPARSE_EVAL_CHUNK=4` builds the other for a timing (tools/gpu_verify_multi_time.py).
#ifndef VDF_SPARSE_EVAL_CHUNK
#define VDF_SPARSE_EVAL_CHUNK 2
#endif
constexpr int SPARSE_EVAL_CHUNK = VDF_SPARSE_EVAL_CHUNK;
static_assert(SPARSE_EVAL_CHUNK == 2 || SPARSE_EVAL_CHUNK == 4, "8 instances per pass spill");
template <class P>
__device__ __forceinline__ Fe<P> eval_term(const Fe<P>& ex, const Fe<P> s[3], const EvalItem& it) {
  Fe<P> rho, rho2;
#pragma unroll
  for (int k = 0; k < 8; ++k) { rho.v[k] = it.rho[k]; rho2.v[k] = it.rho2[k]; }
  return fe_mul(ex, fe_add(s[0], fe_add(fe_mul(rho, s[1]), fe_mul(rho2, s[2]))));
}
template <class P, int CH>
__global__ __launch_bounds__(256) void k_sparse_eval_multi(Csr3 m, const char* __restrict__ dict, const EvalItem* __restrict__ items, int count,
                                                           size_t rows, size_t col_split, size_t col_hi_base,
                                                           const uint32_t* __restrict__ long_rowlist, size_t n_long, uint32_t long_wgs,
                                                           char* __restrict__ partials) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  __shared__ uint32_t red[4][CH][8];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool long_wg = blockIdx.x < long_wgs;                       // uniform: a workgroup takes long rows or short ones
  auto ycol = [&](uint32_t c) -> size_t { return c < col_split ? (size_t)c : col_hi_base + ((size_t)c - col_split); };
  // no lane leaves before the last barrier: one without a row (the grid's tail, a long row among the short, a wavefront past
  // the long-row list) carries zero terms
  bool active;
  size_t r = 0;
  if (long_wg) {
    const size_t w = (size_t)blockIdx.x * 4 + wave;
    active = w < n_long;
    if (active) r = long_rowlist[w];
  } else {
    r = (size_t)(blockIdx.x - long_wgs) * 256 + threadIdx.x;
    active = r < rows;
  }
  uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (active) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = m.rowptr[k][r]; hi[k] = m.rowptr[k][r + 1]; }
  }
  if (!long_wg && (hi[0] - lo[0] > VDF_LONG_ROW || hi[1] - lo[1] > VDF_LONG_ROW || hi[2] - lo[2] > VDF_LONG_ROW)) active = false;   // a wavefront's row
  constexpr int PRE[3] = {2, 2, 4};
  size_t cc[3][4];
  uint32_t kk[3][4];
  Fe<P> dv[3][4];
  if (!long_wg) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < PRE[k]; ++j) {
        const bool has = active && lo[k] + j < hi[k];                  // (an absent entry gathers element 0 and is not used)
        cc[k][j] = has ? ycol(m.col[k][lo[k] + j]) : 0;
        kk[k][j] = has ? m.coef[k][lo[k] + j] : 0u;
      }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < PRE[k]; ++j) dv[k][j] = kk[k][j] > 1 ? fe_load<P>(dict + (size_t)kk[k][j] * 32) : fe_zero<P>();
  }
  for (int q0 = 0; q0 < count; q0 += CH) {
    Fe<P> acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      acc[c] = fe_zero<P>();
      if (q0 + c >= count || !active) continue;
      const EvalItem& it = items[q0 + c];
      const Fe<P> ex = fe_load<P>(it.ex + r * 32);
      Fe<P> s[3];
      if (long_wg) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          s[k] = fe_zero<P>();
          for (uint32_t e = lo[k] + lane; e < hi[k]; e += 64)
            s[k] = fe_add(s[k], spmv_term<P>(fe_load<P>(it.ey + ycol(m.col[k][e]) * 32), m.coef[k][e], dict));
        }
      } else {
        Fe<P> v[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int j = 0; j < PRE[k]; ++j) v[k][j] = fe_load<P>(it.ey + cc[k][j] * 32);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          s[k] = fe_zero<P>();
#pragma unroll
          for (int j = 0; j < PRE[k]; ++j) {
            if (lo[k] + j >= hi[k]) break;
            const uint32_t ci = kk[k][j];
            s[k] = ci == 0 ? fe_add(s[k], v[k][j]) : ci == 1 ? fe_sub(s[k], v[k][j]) : fe_add(s[k], fe_mul(v[k][j], dv[k][j]));
          }
          for (uint32_t e = lo[k] + PRE[k]; e < hi[k]; ++e)
            s[k] = fe_add(s[k], spmv_term<P>(fe_load<P>(it.ey + ycol(m.col[k][e]) * 32), m.coef[k][e], dict));
        }
      }
      acc[c] = eval_term<P>(ex, s, it);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (q0 + c >= count) continue;                                   // uniform
      const Fe<P> t = fe_group_sum<P, 64>(acc[c]);
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[wave][c][i] = t.v[i];
      }
    }
    __syncthreads();
    if (threadIdx.x < CH && q0 + (int)threadIdx.x < count) {
      Fe<P> t = fe_zero<P>();
      for (int w = 0; w < 4; ++w) {
        Fe<P> o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = red[w][threadIdx.x][i];
        t = fe_add(t, o);
      }
      fe_store<P>(partials + ((size_t)(q0 + threadIdx.x) * gridDim.x + blockIdx.x) * 32, t);
    }
    __syncthreads();                                                   // the next pass writes red again
  }
}
// out[q] = the sum of instance q's partials: one wavefront per instance
template <class P>
__global__ __launch_bounds__(64) void k_sparse_eval_sum(const char* __restrict__ partials, uint32_t nwg, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);
  const uint32_t q = blockIdx.x, lane = threadIdx.x;
  Fe<P> acc = fe_zero<P>();
  for (uint32_t w = lane; w < nwg; w += 64) acc = fe_add(acc, fe_load<P>(partials + ((size_t)q * nwg + w) * 32));
  acc = fe_group_sum<P, 64>(acc);
  if (lane == 0) fe_store<P>(out + (size_t)q * 32, acc);
}

size_t sparse_eval_item_bytes() { return sizeof(EvalItem); }
// workgroups of a launch over `rows` rows; every instance keeps one 32-byte partial per workgroup
size_t sparse_eval_workgroups(size_t rows, size_t n_long_rows) { return (rows + 255) / 256 + (n_long_rows + 3) / 4; }
Status sparse_eval_pack(int field, int count, const void* const ex[], const void* const ey[], const vdf_fe rho[], void* block) {
  EvalItem* it = reinterpret_cast<EvalItem*>(block);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    for (int q = 0; q < count; ++q) {
      it[q].ex = cbytes_of(ex[q]);
      it[q].ey = cbytes_of(ey[q]);
      Fe<P> r;
      memcpy(r.v, rho[q].l, 32);
      const Fe<P> r2 = fe_sqr(r);
      memcpy(it[q].rho, r.v, 32);
      memcpy(it[q].rho2, r2.v, 32);
    }
    return Status{};
  });
}
// partials: sparse_eval_workgroups() x count elements; d_out: count elements
Status vec_sparse_eval_multi(int field, const uint32_t* const rowptr[3], const uint32_t* const col[3], const uint32_t* const coef[3],
                             const void* dict, const void* block, int count, size_t rows, size_t col_split, size_t col_hi_base,
                             const uint32_t* long_rowlist, size_t n_long_rows, void* partials, void* d_out, double alg_bytes,
                             hipStream_t s) {
  if (count == 0) return Status{};
  Csr3 m;
  for (int k = 0; k < 3; ++k) { m.rowptr[k] = rowptr[k]; m.col[k] = col[k]; m.coef[k] = coef[k]; }
  if (!long_rowlist) n_long_rows = 0;
  const size_t wgs = sparse_eval_workgroups(rows, n_long_rows);
  if (wgs >= ((size_t)1 << 31)) return Status{VDF_ERR_BAD_LENGTH, "shape too large"};
  if (wgs == 0) return hip_status(hipMemsetAsync(d_out, 0, (size_t)count * 32, s), "hipMemsetAsync");     // no rows: every sum is empty
  const uint32_t long_wgs = (uint32_t)((n_long_rows + 3) / 4);
  KTimer kt(s, "k_sparse_eval_multi", alg_bytes);        // both launches: the sum of the partials is part of the evaluation
  VDF_TRY(with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_sparse_eval_multi<tag_t<decltype(f)>, SPARSE_EVAL_CHUNK>), dim3((unsigned)wgs), dim3(256), 0, s, m, cbytes_of(dict),
                       reinterpret_cast<const EvalItem*>(block), count, rows, col_split, col_hi_base, long_rowlist, n_long_rows, long_wgs,
                       bytes_of(partials));
  }));
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_sparse_eval_sum<tag_t<decltype(f)>>), dim3((unsigned)count), dim3(64), 0, s, cbytes_of(partials), (uint32_t)wgs, bytes_of(d_out));
  });
}

// flag |= 1 when any of the n 32-byte elements is not all-zero (a residual vector checked where it lies)
__global__ __launch_bounds__(256) void k_any_nonzero(const uint4* __restrict__ v, size_t n16, uint32_t* __restrict__ flag) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t any = 0;
  for (size_t k = i; k < n16; k += (size_t)gridDim.x * 256) { const uint4 w = v[k]; any |= w.x | w.y | w.z | w.w; }
  if (__any(any != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
Status vec_any_nonzero(const void* v, size_t n, uint32_t* d_flag, hipStream_t s) {
  VDF_TRY_HIP(hipMemsetAsync(d_flag, 0, 4, s));
  if (n == 0) return Status{};
  const size_t n16 = n * 2;
  size_t blocks = (n16 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_any_nonzero, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(v), n16, d_flag);
  VDF_TRY_HIP(hipGetLastError());
  return Status{};
}

// Which rows of an instance are unsatisfied (include/vdf_hip.h vdf_unsat_rows): one row per lane, res[0] += the rows with
// a b != c, res[1] = the smallest of them.  A wavefront with a mismatch sends one lane, its first mismatching one, to the two atomics.
template <class P>
__global__ __launch_bounds__(256) void k_unsat_rows(const char* __restrict__ a, const char* __restrict__ b, const char* __restrict__ c, size_t n,
                                                    unsigned long long* __restrict__ res) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < n) bad = !fe_eq(fe_mul(fe_load<P>(a + i * 32), fe_load<P>(b + i * 32)), fe_load<P>(c + i * 32));
  const unsigned long long m = __ballot(bad);
  if (m != 0 && (int)(threadIdx.x & 63) == __ffsll(m) - 1) {
    atomicAdd(&res[0], (unsigned long long)__popcll(m));
    atomicMin(&res[1], (unsigned long long)i);
  }
}
// d_res: 16 bytes of device memory, initialised here to {0, 2^64 - 1}
Status vec_unsat_rows(int field, const void* a, const void* b, const void* c, size_t n, void* d_res, hipStream_t s) {
  VDF_TRY_HIP(hipMemsetAsync(d_res, 0, 8, s));
  VDF_TRY_HIP(hipMemsetAsync(bytes_of(d_res) + 8, 0xff, 8, s));
  if (n == 0) return Status{};
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_unsat_rows<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, cbytes_of(a), cbytes_of(b), cbytes_of(c), n,
                       reinterpret_cast<unsigned long long*>(d_res));
  });
}

Status vec_mul(int field, const void* a, const void* b, size_t n, void* out, hipStream_t s) {
  if (n == 0) return Status{};
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_mul<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, cbytes_of(a), cbytes_of(b), n, bytes_of(out));
  });
}

Status vec_to_mont(int field, const void* a, size_t n, void* out, hipStream_t s) {
  if (n == 0) return Status{};
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_mont<tag_t<decltype(f)>, 1>), grid_for(n), dim3(256), 0, s, cbytes_of(a), n, bytes_of(out));
  });
}

Status vec_from_mont(int field, const void* a, size_t n, void* out, hipStream_t s) {
  if (n == 0) return Status{};
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_mont<tag_t<decltype(f)>, 0>), grid_for(n), dim3(256), 0, s, cbytes_of(a), n, bytes_of(out));
  });
}

Status vec_mul_chain(int field, const void* a, size_t n, int iters, void* out, hipStream_t s) {
  if (n == 0) return Status{};
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_mul_chain<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, cbytes_of(a), n, iters, bytes_of(out));
  });
}

Status vec_clock_probe(int iters, int workgroups, unsigned long long* d_out3, hipStream_t s) {
  hipLaunchKernelGGL(k_clock_probe, dim3(workgroups), dim3(256), 0, s, iters, d_out3);
  VDF_TRY_HIP(hipGetLastError());
  return Status{};
}

// ---- folding two RELAXED instances (vdf_nova_compress_aggregate) ----------------------------------------------------------------
// The cross term when neither instance is fresh: T = Az1 o Bz2 + Az2 o Bz1 - u1 Cz2 - u2 Cz1 (k_cross_term is the case u2 = 1, and
// gives the same bytes there: every value is canonical).  One row per lane over contiguous 32-byte elements; u1 and u2 travel as
// kernel arguments.
template <class P>
__global__ __launch_bounds__(256) void k_cross_term_relaxed(const char* __restrict__ az1, const char* __restrict__ bz1,
                                                            const char* __restrict__ cz1, FeVal u1, const char* __restrict__ az2,
                                                            const char* __restrict__ bz2, const char* __restrict__ cz2, FeVal u2,
                                                            size_t n, char* __restrict__ T) {
  __builtin_amdgcn_s_setprio(3);     // light kernel: do not starve behind a co-running k_accumulate
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Fe<P> a1 = fe_load<P>(az1 + i * 32), b1 = fe_load<P>(bz1 + i * 32), c1 = fe_load<P>(cz1 + i * 32);
  const Fe<P> a2 = fe_load<P>(az2 + i * 32), b2 = fe_load<P>(bz2 + i * 32), c2 = fe_load<P>(cz2 + i * 32);
  Fe<P> t = fe_add(fe_mul(a1, b2), fe_mul(a2, b1));
  t = fe_sub(t, fe_mul(fe_from_val<P>(u1), c2));
  t = fe_sub(t, fe_mul(fe_from_val<P>(u2), c1));
  fe_store<P>(T + i * 32, t);
}

// The fold that goes with it, in place on the index-1 vectors and in one pass over the rows:
//   Az1 += r Az2, Bz1 += r Bz2, Cz1 += r Cz2 (A z, B z, C z are linear in z: the accumulator's products stay current),
//   E1 += r T + r^2 E2.
// r and r^2 are Montgomery forms made on the host.  Nine vectors read and four written per row.
template <class P>
__global__ __launch_bounds__(256) void k_fold_relaxed(FeVal rv, FeVal r2v, size_t n, char* __restrict__ az1, char* __restrict__ bz1,
                                                      char* __restrict__ cz1, char* __restrict__ e1, const char* __restrict__ az2,
                                                      const char* __restrict__ bz2, const char* __restrict__ cz2,
                                                      const char* __restrict__ e2, const char* __restrict__ T) {
  __builtin_amdgcn_s_setprio(3);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Fe<P> r = fe_from_val<P>(rv), r2 = fe_from_val<P>(r2v);
  fe_store<P>(az1 + i * 32, fe_add(fe_load<P>(az1 + i * 32), fe_mul(r, fe_load<P>(az2 + i * 32))));
  fe_store<P>(bz1 + i * 32, fe_add(fe_load<P>(bz1 + i * 32), fe_mul(r, fe_load<P>(bz2 + i * 32))));
  fe_store<P>(cz1 + i * 32, fe_add(fe_load<P>(cz1 + i * 32), fe_mul(r, fe_load<P>(cz2 + i * 32))));
  const Fe<P> e = fe_add(fe_load<P>(e1 + i * 32), fe_mul(r, fe_load<P>(T + i * 32)));
  fe_store<P>(e1 + i * 32, fe_add(e, fe_mul(r2, fe_load<P>(e2 + i * 32))));
}

Status vec_cross_term_relaxed(int field, const void* az1, const void* bz1, const void* cz1, const vdf_fe* u1, const void* az2,
                              const void* bz2, const void* cz2, const vdf_fe* u2, size_t n, void* T, hipStream_t s) {
  if (n == 0) return Status{};
  if (n >= ((size_t)1 << 39)) return Status{VDF_ERR_BAD_LENGTH, "cross term too large"};
  KTimer kt(s, "k_cross_term_relaxed", 224.0 * n);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_cross_term_relaxed<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, cbytes_of(az1), cbytes_of(bz1),
                       cbytes_of(cz1), to_val(u1), cbytes_of(az2), cbytes_of(bz2), cbytes_of(cz2), to_val(u2), n, bytes_of(T));
  });
}

Status vec_fold_relaxed(int field, const vdf_fe* r, size_t n, void* az1, void* bz1, void* cz1, void* e1, const void* az2,
                        const void* bz2, const void* cz2, const void* e2, const void* T, hipStream_t s) {
  if (n == 0) return Status{};
  if (n >= ((size_t)1 << 39)) return Status{VDF_ERR_BAD_LENGTH, "fold too large"};
  KTimer kt(s, "k_fold_relaxed", 13 * 32.0 * n);
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    Fe<P> rm; std::memcpy(rm.v, r, 32);
    const Fe<P> rr = fe_mul(rm, rm);                  // r^2, once, on the host
    FeVal r2v; std::memcpy(r2v.v, rr.v, 32);
    hipLaunchKernelGGL((k_fold_relaxed<P>), grid_for(n), dim3(256), 0, s, to_val(r), r2v, n, bytes_of(az1), bytes_of(bz1), bytes_of(cz1),
                       bytes_of(e1), cbytes_of(az2), cbytes_of(bz2), cbytes_of(cz2), cbytes_of(e2), cbytes_of(T));
  });
}

// ---- the random oracle, family 0 (vdf_ro_hash_batch) ----------------------------------------------------------------------------
// host/r1cs.cpp ro_hash / ro_permute restated one message per lane: width 4, rate 3, x^5, 8 external and 56 internal rounds.
// The state is four NAMED elements (a run-time lane index would put it in scratch); every value between two S-boxes is
// canonical (fe_add), and inside an S-box the three products are lazy: x < m gives x^2 < 2m + eps, x^4 < 2m + 2 eps,
// x^5 < 2m + 3 eps < 3m (fe.cuh, "lazy domain"), which fe_canon's two conditional subtractions bring below m.
template <class P> __device__ __forceinline__ Fe<P> ro_sbox(const Fe<P>& x) {
  const Fe<P> x2 = fe_sqr_lazy(x);
  const Fe<P> x4 = fe_sqr_lazy(x2);
  return fe_canon(fe_mul_lazy(x4, x));
}
// M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]] with 14 additions (ext_layer)
template <class P> __device__ __forceinline__ void ro_ext_layer(Fe<P>& a, Fe<P>& b, Fe<P>& c, Fe<P>& d) {
  const Fe<P> t0 = fe_add(a, b), t1 = fe_add(c, d);
  const Fe<P> t2 = fe_add(fe_dbl(b), t1), t3 = fe_add(fe_dbl(d), t0);
  const Fe<P> t4 = fe_add(fe_dbl(fe_dbl(t1)), t3), t5 = fe_add(fe_dbl(fe_dbl(t0)), t2);
  a = fe_add(t3, t5); b = t5; c = fe_add(t2, t4); d = t4;
}
// ones off the diagonal, (2, 3, 6, 8) on it: s_i <- sum + (1, 2, 5, 7)_i s_i (int_layer); no products
template <class P> __device__ __forceinline__ void ro_int_layer(Fe<P>& a, Fe<P>& b, Fe<P>& c, Fe<P>& d) {
  const Fe<P> tot = fe_add(fe_add(a, b), fe_add(c, d));
  const Fe<P> c4 = fe_dbl(fe_dbl(c)), d8 = fe_dbl(fe_dbl(fe_dbl(d)));
  a = fe_add(tot, a);
  b = fe_add(tot, fe_dbl(b));
  c = fe_add(tot, fe_add(c4, c));
  d = fe_add(tot, fe_sub(d8, d));
}
// rc: VDF_RO_CONSTANTS elements, ext[r][lane] for r = 0..7 and then in[0..55].  The index of every constant is the loop counter,
// the same in every lane, so the constants travel through scalar loads.  The rounds are three loops (4 + 56 + 4) in one outer
// loop of two trips, so that the external round's four S-boxes exist once in the code.
template <class P> __device__ __forceinline__ void ro_permute_dev(Fe<P>& a, Fe<P>& b, Fe<P>& c, Fe<P>& d, const char* __restrict__ rc) {
  ro_ext_layer(a, b, c, d);
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
#pragma unroll 1
    for (int r = 0; r < 4; ++r) {
      const char* k = rc + (size_t)(half * 4 + r) * 128;
      a = ro_sbox(fe_add(a, fe_load<P>(k)));
      b = ro_sbox(fe_add(b, fe_load<P>(k + 32)));
      c = ro_sbox(fe_add(c, fe_load<P>(k + 64)));
      d = ro_sbox(fe_add(d, fe_load<P>(k + 96)));
      ro_ext_layer(a, b, c, d);
    }
    if (half == 0) {
#pragma unroll 1
      for (int r = 0; r < 56; ++r) {
        a = ro_sbox(fe_add(a, fe_load<P>(rc + (size_t)(32 + r) * 32)));
        ro_int_layer(a, b, c, d);
      }
    }
  }
}
// out[i] = ro_hash(tag, xs + i len, len): lane 0 starts as s0 = tag + (len << 32) in Montgomery form (made by the launcher),
// each block of three elements is added into lanes 1..3 and followed by one permutation, the result is lane 1.  len, bits and
// every constant index are wave-uniform: no loop, branch or address depends on a message.  bits = 0 stores the Montgomery
// form; otherwise the canonical integer's low `bits` bits as a plain integer.
template <class P>
__global__ __launch_bounds__(256) void k_ro_hash(const char* __restrict__ rc, const char* __restrict__ xs, uint32_t len, uint32_t n,
                                                 FeVal s0, int bits, char* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fe<P> a = fe_from_val<P>(s0), b = fe_zero<P>(), c = fe_zero<P>(), d = fe_zero<P>();
  const char* x = xs + (size_t)i * len * 32;
#pragma unroll 1
  for (uint32_t k = 0; k < len; k += 3) {
    b = fe_add(b, fe_load<P>(x + (size_t)k * 32));
    if (k + 1 < len) c = fe_add(c, fe_load<P>(x + (size_t)(k + 1) * 32));
    if (k + 2 < len) d = fe_add(d, fe_load<P>(x + (size_t)(k + 2) * 32));
    ro_permute_dev(a, b, c, d, rc);
  }
  if (bits != 0) {
    b = fe_from_mont(b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int keep = bits - 32 * j;
      b.v[j] &= keep >= 32 ? 0xFFFFFFFFu : (keep <= 0 ? 0u : (1u << keep) - 1u);
    }
  }
  fe_store<P>(out + (size_t)i * 32, b);
}

Status ro_hash_batch(int field, uint64_t tag, const void* d_rc, const void* d_xs, size_t len, size_t n, int bits, void* d_out,
                     hipStream_t s) {
  VDF_TRY(check_field(field));
  if (bits < 0 || bits > 255) return Status{VDF_ERR_BAD_ARG, "bits must be 0 (the element) or 1..255"};
  if (len > VDF_RO_HASH_MAX_LEN) return Status{VDF_ERR_BAD_ARG, "at most VDF_RO_HASH_MAX_LEN elements per message"};
  if (n == 0) return Status{};
  if (n > 0xFFFFFFFFull) return Status{VDF_ERR_BAD_LENGTH, "at most 2^32 - 1 messages per call"};
  KTimer kt(s, "k_ro_hash", 32.0 * n * (len + 1));
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    const Fe<P> s0 = fe_from_u64<P>(tag + ((uint64_t)len << 32));
    FeVal s0v; std::memcpy(s0v.v, s0.v, 32);
    hipLaunchKernelGGL((k_ro_hash<P>), grid_for(n), dim3(256), 0, s, cbytes_of(d_rc), cbytes_of(d_xs), (uint32_t)len, (uint32_t)n, s0v, bits,
                       bytes_of(d_out));
  });
}

// ---- the random oracle, family 1 (vdf_ro_hash_batch_block) ----------------------------------------------------------------------
// host/r1cs.cpp ro_hash / classic_permute restated for a non-default block (width t <= 25, rf full and rp partial rounds, dense
// t x t matrix), one message per 32 consecutive lanes: lane i < t of a group owns state element i in registers, so no lane
// holds an array indexed at run time.  A round adds rc[r t + i] (loaded during the round before), applies x^5 (every lane in a
// full round, lane 0 otherwise: a per-lane select on a wave-uniform flag), and then s_i <- sum_j M[i][j] s_j: every lane
// publishes its element in its message's LDS slots and reads all t back -- the 32 lanes of a group read ONE address, which
// broadcasts.
//
// LDS: M once per workgroup, transposed and split into two planes of 16-byte halves, sM[half][j * 32 + i]: for a fixed j the
// lanes of a group read consecutive 16-byte slots (dword 4 i, 64 banks: the 16 lanes of every ds_read_b128 lane group fall on 16
// distinct bank quads), and lanes i and i + 32 read the same address.  Rows i >= t of both planes are zero, so an idle lane's
// element stays zero.  The slots are double-buffered on the round's parity: a lane writes buffer p, passes the round's one
// barrier and reads buffer p; the next write to p is two rounds later, behind the next round's barrier, which no wavefront
// passes before every reader of p has arrived at it.
//
// Every wavefront runs every loop and every barrier: groups past n and lanes >= t skip only global loads and stores.  Trip
// counts, branches and addresses come from the kernel arguments and the lane index, never from a message.  Every value kept
// between two operations is canonical (fe_add, fe_mul_inl; ro_sbox ends in fe_canon), so the result is ro_hash's mod m.
constexpr int RO_BLOCK_MAX_T = 25;
static_assert(RO_BLOCK_MAX_T == VDF_RO_BLOCK_MAX_WIDTH && RO_BLOCK_MAX_T <= 32, "one state element per lane of a 32-lane group");
template <class P>
__global__ __launch_bounds__(256) void k_ro_hash_block(const char* __restrict__ rc, const char* __restrict__ mds, const char* __restrict__ xs,
                                                       uint32_t len, uint32_t n, uint32_t t, uint32_t rf, uint32_t rp, FeVal s0, int bits,
                                                       char* __restrict__ out) {
  __shared__ uint4 sM[2][RO_BLOCK_MAX_T * 32];         // [half][column j][row i]
  __shared__ uint4 sS[2][8][32][2];                    // [parity][message of the workgroup][element][half]
  const uint32_t g = threadIdx.x >> 5, i = threadIdx.x & 31;
  const uint32_t msg = blockIdx.x * 8 + g;
  const bool mine = i < t, live = mine && msg < n;     // live: this lane may touch global memory
  for (uint32_t e = threadIdx.x; e < t * 32; e += 256) {
    const uint32_t j = e >> 5, row = e & 31;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (row < t) {
      const uint4* q = reinterpret_cast<const uint4*>(mds + ((size_t)row * t + j) * 32);
      lo = q[0]; hi = q[1];
    }
    sM[0][e] = lo; sM[1][e] = hi;
  }
  __syncthreads();
  Fe<P> s = i == 0 ? fe_from_val<P>(s0) : fe_zero<P>();
  const uint32_t rate = t - 1, half = rf / 2, rounds = rf + rp;
  uint32_t par = 0;
  Fe<P> c = fe_zero<P>();                              // the round's constant, loaded one round ahead (an idle lane's stays zero)
  if (live) c = fe_load<P>(rc + (size_t)i * 32);
#pragma unroll 1
  for (uint32_t k = 0; k < len; k += rate) {
    // lane i >= 1 absorbs element k + (i - 1) of its message; lane 0 absorbs nothing (and its i - 1 is never formed)
    const uint32_t idx = i >= 1 ? k + (i - 1) : len;
    if (live && idx < len) s = fe_add(s, fe_load<P>(xs + ((size_t)msg * len + idx) * 32));
#pragma unroll 1
    for (uint32_t r = 0; r < rounds; ++r) {
      s = fe_add(s, c);
      const Fe<P> s5 = ro_sbox(s);
      const bool box = r < half || r >= half + rp || i == 0;
#pragma unroll
      for (int w = 0; w < 8; ++w) s.v[w] = box ? s5.v[w] : s.v[w];
      sS[par][g][i][0] = make_uint4(s.v[0], s.v[1], s.v[2], s.v[3]);
      sS[par][g][i][1] = make_uint4(s.v[4], s.v[5], s.v[6], s.v[7]);
      // the next round's constant does not depend on the state: its load is issued here and lands during the matrix loop.  After
      // the last round that is round 0 again, which the next block's permutation begins with (and which is in range at the end).
      const uint32_t rn = r + 1 < rounds ? r + 1 : 0;
      if (live) c = fe_load<P>(rc + ((size_t)rn * t + i) * 32);
      __syncthreads();
      Fe<P> acc = fe_zero<P>();
#pragma unroll 1
      for (uint32_t j = 0; j < t; ++j) {
        const uint4 ml = sM[0][j * 32 + i], mh = sM[1][j * 32 + i], vl = sS[par][g][j][0], vh = sS[par][g][j][1];
        Fe<P> m, v;
        m.v[0] = ml.x; m.v[1] = ml.y; m.v[2] = ml.z; m.v[3] = ml.w; m.v[4] = mh.x; m.v[5] = mh.y; m.v[6] = mh.z; m.v[7] = mh.w;
        v.v[0] = vl.x; v.v[1] = vl.y; v.v[2] = vl.z; v.v[3] = vl.w; v.v[4] = vh.x; v.v[5] = vh.y; v.v[6] = vh.z; v.v[7] = vh.w;
        acc = fe_add(acc, fe_mul_inl(m, v));
      }
      s = acc;
      par ^= 1;
    }
  }
  if (bits != 0) {
    s = fe_from_mont(s);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int keep = bits - 32 * j;
      s.v[j] &= keep >= 32 ? 0xFFFFFFFFu : (keep <= 0 ? 0u : (1u << keep) - 1u);
    }
  }
  if (live && i == 1) fe_store<P>(out + (size_t)msg * 32, s);
}

Status ro_block_shape(int width, int full_rounds, int partial_rounds) {
  if (width < 2 || width > VDF_RO_BLOCK_MAX_WIDTH) return Status{VDF_ERR_BAD_ARG, "width must be 2..VDF_RO_BLOCK_MAX_WIDTH"};
  if (full_rounds < 2 || full_rounds > VDF_RO_BLOCK_MAX_FULL || (full_rounds & 1))
    return Status{VDF_ERR_BAD_ARG, "full_rounds must be even and 2..VDF_RO_BLOCK_MAX_FULL"};
  if (partial_rounds < 0 || partial_rounds > VDF_RO_BLOCK_MAX_PARTIAL) return Status{VDF_ERR_BAD_ARG, "partial_rounds must be 0..VDF_RO_BLOCK_MAX_PARTIAL"};
  return Status{};
}

Status ro_hash_batch_block(int field, uint64_t tag, int width, int full_rounds, int partial_rounds, const void* d_rc, const void* d_mds,
                           const void* d_xs, size_t len, size_t n, int bits, void* d_out, hipStream_t s) {
  VDF_TRY(check_field(field));
  VDF_TRY(ro_block_shape(width, full_rounds, partial_rounds));
  if (bits < 0 || bits > 255) return Status{VDF_ERR_BAD_ARG, "bits must be 0 (the element) or 1..255"};
  if (len > VDF_RO_HASH_MAX_LEN) return Status{VDF_ERR_BAD_ARG, "at most VDF_RO_HASH_MAX_LEN elements per message"};
  if (n == 0) return Status{};
  if (n > 0xFFFFFFFFull) return Status{VDF_ERR_BAD_LENGTH, "at most 2^32 - 1 messages per call"};
  KTimer kt(s, "k_ro_hash_block", 32.0 * n * (len + 1));
  return with_field(field, [&](auto f) {
    using P = tag_t<decltype(f)>;
    const Fe<P> s0 = fe_from_u64<P>(tag + ((uint64_t)len << 32));
    FeVal s0v; std::memcpy(s0v.v, s0.v, 32);
    hipLaunchKernelGGL((k_ro_hash_block<P>), dim3((unsigned)((n + 7) / 8)), dim3(256), 0, s, cbytes_of(d_rc), cbytes_of(d_mds), cbytes_of(d_xs),
                       (uint32_t)len, (uint32_t)n, (uint32_t)width, (uint32_t)full_rounds, (uint32_t)partial_rounds, s0v, bits, bytes_of(d_out));
  });
}

}  // namespace vdf
