// Kernels of the compression SNARK (protocol "vdf-spartan-v3", restated by the test oracle, spartan.py): a Spartan-style
// argument for the folded relaxed R1CS instance with inner-product-argument openings -- the work behind
// `NovaVDFProof::compress` / verification of the compressed proof (/root/reference/src/nova/proof.rs:360-368, :383;
// nova-snark 0.8.0 `CompressedSNARK`).
//
// Everything here is a streaming pass or a reduction over vectors of field elements: HBM-bound, no MFMA.
// Multilinear tables are MSB-first (index i = sum x_j 2^(k-j)): binding a variable folds the upper half of a table
// onto its lower half, so every pass reads two coalesced halves.
//   k_eq_table        out[i] = prod_j (bit_j(i) ? hi_j : lo_j)   (eq(r, .) with lo = 1 - r, hi = r)
//   k_ipa_coefficients  out[i] = sum_q w_q pattern_q[low bits of i] prod_j (bit_j ? hi_qj : lo_qj): the inner-product
//                     argument's generator coefficients (lo = x^-1, hi = x) of one opening, or a weighted sum over many
//   k_fold_halves     v[i] <- c_lo v[i] + c_hi v[i + h] for up to 8 vectors (sum-check binding: c = (1 - r, r);
//                     inner-product argument: (x, x^-1) / (x^-1, x))
//   k_reduce / k_reduce_final   sums over i < h of a per-kind term (dot product, the two sum-check round
//                     polynomials at their evaluation points, the argument's cross terms); per-workgroup LDS tree,
//                     then one workgroup over the partials
//   k_spmvt / k_spmvt_heavy     M(y) = sum_x eq[x] (A + rho B + rho^2 C)[x, y]: the three matrices merged in column-major
//                     order; a thread per column, a workgroup per heavy column (the constant column has ~t entries)
//   k_ipa_scalars     the two scalar vectors whose MSMs over the ORIGINAL generators are a round's L and R
//   k_scale_pattern   s[t] *= ((t mod n_j) >= n_j / 2) ? x : x^-1
//   k_reduce_batch / k_fold_halves_batch / k_spmvt_batch   the same passes for many instances of one length at once (the
//                     lockstep rounds of several proofs: one launch with K times the rows, not K launches)
#include <cstring>
#include "internal.h"
#include "fe.cuh"

namespace vdf {

struct FeArg { uint32_t v[8]; };
template <class P> __device__ __forceinline__ Fe<P> arg_fe(const FeArg& a) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = a.v[i];
  return r;
}
static FeArg to_arg(const vdf_fe* p) { FeArg v; std::memcpy(v.v, p, 32); return v; }

// ---- tensor-product tables ---------------------------------------------------------------------------
struct PairArgs { FeArg lo[24], hi[24]; int k; };

template <class P>
__global__ __launch_bounds__(256) void k_eq_table(PairArgs a, size_t n, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fe<P> acc = fe_one<P>();
  for (int j = 0; j < a.k; ++j) {
    const bool bit = (i >> (a.k - 1 - j)) & 1;               // variable j is bit k-1-j of the index (x_1 = MSB)
    acc = fe_mul(acc, arg_fe<P>(bit ? a.hi[j] : a.lo[j]));
  }
  fe_store<P>(out + i * 32, acc);
}

Status snark_pair_table(int field, const vdf_fe* lo, const vdf_fe* hi, int k, void* out, hipStream_t s) {
  if (k < 0 || k > 24) return Status{VDF_ERR_BAD_LENGTH, "at most 24 variables"};
  PairArgs a{};
  a.k = k;
  for (int j = 0; j < k; ++j) { a.lo[j] = to_arg(&lo[j]); a.hi[j] = to_arg(&hi[j]); }
  const size_t n = (size_t)1 << k;
  KTimer kt(s, "k_eq_table", 32.0 * n);                          // one element written per index; the factors are kernel arguments
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_eq_table<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, a, n, bytes_of(out));
  });
}

// ---- the inner-product argument's generator coefficients, for many openings at once ------------------------------
// out[i] = sum over openings q with i < 2^(k_q + log_m_q) of
//            w_q * pattern_q[i mod 2^log_m_q] * prod_j (bit (k_q-1-j) of (i >> log_m_q) ? hi_q[j] : lo_q[j])
// -- the coefficient of generator i in a weighted sum of verifier checks of arguments that stopped at a vector of 2^log_m
// elements (one opening with w = 1: the single check, vdf_pair_table_pattern).  The factors live in a device block
// (IpaOpDev per opening) read at wave-uniform addresses.  Wave v owns the 512 entries [512 v, 512 v + 512), its lane l
// the eight entries 512 v + l + 64 e, e < 8: the index bits that vary within a thread are 6..8, so per opening a thread
// forms the product over every other bit once (the weight and the pattern element folded in) and expands bits 8, 7, 6 as
// a three-level product tree -- 14 products for 8 entries, plus k/8 for the prefix, instead of k per entry; the stores of
// one instruction are 64 consecutive entries.
struct IpaOpDev { FeArg w, lo[24], hi[24], pat[16]; int k, log_m, pad[6]; };
static constexpr int IPA_RUN = 8;                              // entries per thread (index bits 6..8)

size_t snark_ipa_block_bytes(int count) { return (size_t)(count > 0 ? count : 0) * sizeof(IpaOpDev); }

void snark_ipa_pack(const vdf_ipa_opening* ops, int count, void* block) {
  IpaOpDev* d = reinterpret_cast<IpaOpDev*>(block);
  for (int q = 0; q < count; ++q) {
    IpaOpDev o{};
    const vdf_ipa_opening& s = ops[q];
    o.k = s.k; o.log_m = s.log_m;
    o.w = to_arg(&s.weight);
    for (int j = 0; j < s.k; ++j) { o.lo[j] = to_arg(&s.lo[j]); o.hi[j] = to_arg(&s.hi[j]); }
    for (int j = 0; j < (1 << s.log_m); ++j) o.pat[j] = to_arg(&s.pattern[j]);
    std::memcpy(&d[q], &o, sizeof(o));
  }
}

Status snark_field_one(int field, vdf_fe* out) {
  return with_field(field, [&](auto f) {
    const auto one = fe_one<tag_t<decltype(f)>>();
    std::memcpy(out, one.v, 32);
    return Status{};
  });
}

template <class P>
__device__ __forceinline__ Fe<P> pick(const IpaOpDev& o, int j, bool bit) {
  const Fe<P> lo = arg_fe<P>(o.lo[j]), hi = arg_fe<P>(o.hi[j]);      // both uniform loads, a per-lane select
  return bit ? hi : lo;
}

template <class P>
__global__ __launch_bounds__(256) void k_ipa_coefficients(const IpaOpDev* __restrict__ ops, int count, size_t n, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);
  const unsigned lane = threadIdx.x & 63;
  const size_t base = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 * IPA_RUN);      // wave-uniform
  if (base >= n) return;
  const size_t i0 = base + lane;
  Fe<P> acc[IPA_RUN];
#pragma unroll
  for (int e = 0; e < IPA_RUN; ++e) acc[e] = fe_zero<P>();
  for (int q = 0; q < count; ++q) {
    const IpaOpDev& o = ops[q];
    const int k = o.k, log_m = o.log_m, K = k + log_m;          // round variable j is index bit K-1-j
    if (base >> K) continue;                                    // every entry of this wave is past the opening
    const Fe<P> pw = fe_mul(arg_fe<P>(o.w), fe_load<P>(&o.pat[lane & ((1u << log_m) - 1)]));
    if (K >= 9) {                                               // bits 6..8 are round bits: the whole run is inside the opening
      Fe<P> pre = pw;
      for (int j = 0; j < k; ++j) {
        const int b = K - 1 - j;
        if (b >= 6 && b < 9) continue;
        pre = fe_mul(pre, pick<P>(o, j, (i0 >> b) & 1));
      }
      const int j8 = K - 9, j7 = K - 8, j6 = K - 7;
#pragma unroll
      for (int b8 = 0; b8 < 2; ++b8) {
        const Fe<P> s8 = fe_mul(pre, pick<P>(o, j8, b8));
#pragma unroll
        for (int b7 = 0; b7 < 2; ++b7) {
          const Fe<P> s7 = fe_mul(s8, pick<P>(o, j7, b7));
#pragma unroll
          for (int b6 = 0; b6 < 2; ++b6) {
            const int e = 4 * b8 + 2 * b7 + b6;
            acc[e] = fe_add(acc[e], fe_mul(s7, pick<P>(o, j6, b6)));
          }
        }
      }
    } else {                                                    // an opening of fewer than 512 entries (base = 0): entry by entry
#pragma unroll
      for (int e = 0; e < IPA_RUN; ++e) {
        const size_t i = i0 + 64 * e;
        if (i >> K) continue;
        Fe<P> v = pw;
        for (int j = 0; j < k; ++j) v = fe_mul(v, pick<P>(o, j, (i >> (K - 1 - j)) & 1));
        acc[e] = fe_add(acc[e], v);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < IPA_RUN; ++e) {
    const size_t i = i0 + 64 * e;
    if (i < n) fe_store<P>(out + i * 32, acc[e]);
  }
}

Status snark_ipa_coefficients(int field, const void* block, int count, size_t n, void* out, hipStream_t s) {
  if (n == 0) return Status{};
  const size_t waves = (n + 64 * IPA_RUN - 1) / (64 * IPA_RUN);
  const dim3 grid((unsigned)((waves + 3) / 4));
  KTimer kt(s, "k_ipa_coefficients", 32.0 * n);                // one element written per index; the factors are a few KiB
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_ipa_coefficients<tag_t<decltype(f)>>), grid, dim3(256), 0, s, reinterpret_cast<const IpaOpDev*>(block), count, n, bytes_of(out));
  });
}

// ---- folding the two halves of up to 8 vectors ----------------------------------------------------------
struct FoldHalvesArgs { char* v[8]; FeArg c_lo[8], c_hi[8]; int k; };

template <class P>
__global__ __launch_bounds__(256) void k_fold_halves(FoldHalvesArgs a, size_t h) {
  __builtin_amdgcn_s_setprio(3);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= h) return;
  const int t = blockIdx.y;
  char* v = a.v[t];
  const Fe<P> lo = fe_load<P>(v + i * 32), hi = fe_load<P>(v + (h + i) * 32);
  fe_store<P>(v + i * 32, fe_add(fe_mul(arg_fe<P>(a.c_lo[t]), lo), fe_mul(arg_fe<P>(a.c_hi[t]), hi)));
}

Status snark_fold_halves(int field, int k, void* const v[], const vdf_fe c_lo[], const vdf_fe c_hi[], size_t n, hipStream_t s) {
  if (k <= 0) return Status{};
  if (k > 8) return Status{VDF_ERR_BAD_ARG, "at most 8 vectors"};
  if (n < 2 || (n & (n - 1))) return Status{VDF_ERR_BAD_LENGTH, "length must be a power of two >= 2"};
  FoldHalvesArgs a{};
  a.k = k;
  for (int t = 0; t < k; ++t) { a.v[t] = bytes_of(v[t]); a.c_lo[t] = to_arg(&c_lo[t]); a.c_hi[t] = to_arg(&c_hi[t]); }
  const size_t h = n / 2;
  dim3 grid((unsigned)((h + 255) / 256), (unsigned)k);
  KTimer kt(s, "k_fold_halves", 96.0 * h * k);                   // two halves read, the lower one written, per vector
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_fold_halves<tag_t<decltype(f)>>), grid, dim3(256), 0, s, a, h);
  });
}

// ---- reductions ------------------------------------------------------------------------------------------
// kind 0: dot product            sum a[i] b[i], i < n                                   (1 value)
// kind 1: quadratic round        g(0), g(2) of sum (p_lo + t dp)(q_lo + t dq), i < h     (2 values)
// kind 2: cubic R1CS round       g(0), g(2), g(3) of sum eq_t (a_t b_t - u c_t - e_t)    (3 values)
// kind 3: argument cross terms   sum a[i] b[h + i],  sum a[h + i] b[i], i < h            (2 values)
struct ReduceArgs { const char* t[5]; FeArg u; size_t n; };
static constexpr int REDUCE_BLOCKS = 512;

template <class P, int KIND>
__device__ __forceinline__ void reduce_term(const ReduceArgs& a, size_t i, size_t h, Fe<P> acc[3]) {
  if (KIND == 0) {
    acc[0] = fe_add(acc[0], fe_mul(fe_load<P>(a.t[0] + i * 32), fe_load<P>(a.t[1] + i * 32)));
  } else if (KIND == 1) {
    const Fe<P> p0 = fe_load<P>(a.t[0] + i * 32), p1 = fe_load<P>(a.t[0] + (h + i) * 32);
    const Fe<P> q0 = fe_load<P>(a.t[1] + i * 32), q1 = fe_load<P>(a.t[1] + (h + i) * 32);
    acc[0] = fe_add(acc[0], fe_mul(p0, q0));
    const Fe<P> p2 = fe_sub(fe_dbl(p1), p0), q2 = fe_sub(fe_dbl(q1), q0);        // lo + 2 (hi - lo)
    acc[1] = fe_add(acc[1], fe_mul(p2, q2));
  } else if (KIND == 2) {
    const Fe<P> u = arg_fe<P>(a.u);
    Fe<P> lo[5], d[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      lo[k] = fe_load<P>(a.t[k] + i * 32);
      d[k] = fe_sub(fe_load<P>(a.t[k] + (h + i) * 32), lo[k]);
    }
    // t = 0
    acc[0] = fe_add(acc[0], fe_mul(lo[0], fe_sub(fe_sub(fe_mul(lo[1], lo[2]), fe_mul(u, lo[3])), lo[4])));
    // t = 2, then t = 3
    Fe<P> v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = fe_add(lo[k], fe_dbl(d[k]));
    acc[1] = fe_add(acc[1], fe_mul(v[0], fe_sub(fe_sub(fe_mul(v[1], v[2]), fe_mul(u, v[3])), v[4])));
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = fe_add(v[k], d[k]);
    acc[2] = fe_add(acc[2], fe_mul(v[0], fe_sub(fe_sub(fe_mul(v[1], v[2]), fe_mul(u, v[3])), v[4])));
  } else {
    acc[0] = fe_add(acc[0], fe_mul(fe_load<P>(a.t[0] + i * 32), fe_load<P>(a.t[1] + (h + i) * 32)));
    acc[1] = fe_add(acc[1], fe_mul(fe_load<P>(a.t[0] + (h + i) * 32), fe_load<P>(a.t[1] + i * 32)));
  }
}

template <int KIND> struct ReduceOuts { static constexpr int N = KIND == 0 ? 1 : KIND == 2 ? 3 : 2; };

template <class P, int NOUT>
__device__ __forceinline__ void block_tree(Fe<P> acc[3], char* lds) {
  // lds: 256 x NOUT field elements
  for (int k = 0; k < NOUT; ++k) fe_store<P>(lds + ((size_t)k * 256 + threadIdx.x) * 32, acc[k]);
  __syncthreads();
  for (int stride = 128; stride >= 1; stride >>= 1) {
    if ((int)threadIdx.x < stride)
      for (int k = 0; k < NOUT; ++k) {
        char* p = lds + ((size_t)k * 256 + threadIdx.x) * 32;
        fe_store<P>(p, fe_add(fe_load<P>(p), fe_load<P>(p + (size_t)stride * 32)));
      }
    __syncthreads();
  }
}

template <class P, int KIND>
__global__ __launch_bounds__(256) void k_reduce(ReduceArgs a, char* __restrict__ partials) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[256 * 3 * 32];
  constexpr int NOUT = ReduceOuts<KIND>::N;
  const size_t h = KIND == 0 ? a.n : a.n / 2;
  Fe<P> acc[3] = {fe_zero<P>(), fe_zero<P>(), fe_zero<P>()};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < h; i += (size_t)gridDim.x * 256) reduce_term<P, KIND>(a, i, h, acc);
  block_tree<P, NOUT>(acc, lds);
  if (threadIdx.x < NOUT) fe_store<P>(partials + ((size_t)blockIdx.x * NOUT + threadIdx.x) * 32, fe_load<P>(lds + (size_t)threadIdx.x * 256 * 32));
}

template <class P, int NOUT>
__global__ __launch_bounds__(256) void k_reduce_final(const char* __restrict__ partials, int nblocks, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[256 * 3 * 32];
  Fe<P> acc[3] = {fe_zero<P>(), fe_zero<P>(), fe_zero<P>()};
  for (int b = threadIdx.x; b < nblocks; b += 256)
    for (int k = 0; k < NOUT; ++k) acc[k] = fe_add(acc[k], fe_load<P>(partials + ((size_t)b * NOUT + k) * 32));
  block_tree<P, NOUT>(acc, lds);
  if (threadIdx.x < NOUT) fe_store<P>(out + (size_t)threadIdx.x * 32, fe_load<P>(lds + (size_t)threadIdx.x * 256 * 32));
}

template <class P, int KIND>
static Status reduce_launch(const ReduceArgs& a, void* scratch, void* out, hipStream_t s) {
  constexpr int NOUT = ReduceOuts<KIND>::N;
  const size_t h = KIND == 0 ? a.n : a.n / 2;
  int blocks = (int)((h + 255) / 256);
  if (blocks > REDUCE_BLOCKS) blocks = REDUCE_BLOCKS;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL((k_reduce<P, KIND>), dim3(blocks), dim3(256), 0, s, a, bytes_of(scratch));
  hipLaunchKernelGGL((k_reduce_final<P, NOUT>), dim3(1), dim3(256), 0, s, cbytes_of(scratch), blocks, bytes_of(out));
  VDF_TRY_HIP(hipGetLastError());
  return Status{};
}

static constexpr const char* BAD_KIND = "unknown reduction";
size_t snark_reduce_scratch_bytes() { return (size_t)REDUCE_BLOCKS * 3 * 32; }

Status snark_reduce(int field, int kind, const void* const tables[], const vdf_fe* u, size_t n, void* scratch, void* out,
                    hipStream_t s) {
  if (kind < 0 || kind > 3) return Status{VDF_ERR_BAD_ARG, BAD_KIND};
  if (kind != 0 && (n < 2 || (n & (n - 1)))) return Status{VDF_ERR_BAD_LENGTH, "length must be a power of two >= 2"};
  ReduceArgs a{};
  const int ntab = kind == 2 ? 5 : 2;
  for (int k = 0; k < ntab; ++k) a.t[k] = cbytes_of(tables[k]);
  if (u) a.u = to_arg(u);
  a.n = n;
  // bytes read: kind 0 two vectors of n; kind 1 / 3 two vectors of n (both halves); kind 2 five tables of n
  KTimer kt(s, kind == 0 ? "k_reduce(dot)" : kind == 1 ? "k_reduce(quad round)" : kind == 2 ? "k_reduce(cubic round)" : "k_reduce(ipa cross)",
            32.0 * n * ntab);
  return with_field(field, [&](auto f) {
    return with_int<0, 1, 2, 3>(kind, BAD_KIND, [&](auto k) { return reduce_launch<tag_t<decltype(f)>, k.value>(a, scratch, out, s); });
  });
}

// ---- transposed sparse product -----------------------------------------------------------------------------
// Column-major merge of the three matrices: entry = (row, coefficient index | matrix << 30).
static constexpr uint32_t SPMVT_HEAVY = 64;      // columns with more entries than this get a workgroup of their own

template <class P>
__device__ __forceinline__ Fe<P> spmvt_entry(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cm,
                                             const char* __restrict__ dict, const char* __restrict__ eq, const Fe<P> pw[3],
                                             uint32_t k) {
  const uint32_t c = cm[k], ci = c & 0x3FFFFFFFu, mat = c >> 30;
  Fe<P> v = fe_load<P>(eq + (size_t)rows[k] * 32);
  if (ci == 1) v = fe_neg(v);                                   // dictionary index 0 = +1, 1 = -1
  else if (ci > 1) v = fe_mul(v, fe_load<P>(dict + (size_t)ci * 32));
  return mat == 0 ? v : fe_mul(v, pw[mat]);
}

template <class P>
__global__ __launch_bounds__(256) void k_spmvt(const uint32_t* __restrict__ colptr, const uint32_t* __restrict__ rows,
                                               const uint32_t* __restrict__ cm, const char* __restrict__ dict,
                                               const char* __restrict__ eq, FeArg rho, size_t ncols, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= ncols) return;
  const uint32_t lo = colptr[c], hi = colptr[c + 1];
  if (hi - lo > SPMVT_HEAVY) return;                            // k_spmvt_heavy writes this column
  Fe<P> pw[3];
  pw[0] = fe_one<P>(); pw[1] = arg_fe<P>(rho); pw[2] = fe_mul(pw[1], pw[1]);
  Fe<P> acc = fe_zero<P>();
  for (uint32_t k = lo; k < hi; ++k) acc = fe_add(acc, spmvt_entry<P>(rows, cm, dict, eq, pw, k));
  fe_store<P>(out + c * 32, acc);
}

template <class P>
__global__ __launch_bounds__(256) void k_spmvt_heavy(const uint32_t* __restrict__ heavy, const uint32_t* __restrict__ colptr,
                                                     const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cm,
                                                     const char* __restrict__ dict, const char* __restrict__ eq, FeArg rho,
                                                     char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[256 * 3 * 32];
  const uint32_t c = heavy[blockIdx.x];
  const uint32_t lo = colptr[c], hi = colptr[c + 1];
  Fe<P> pw[3];
  pw[0] = fe_one<P>(); pw[1] = arg_fe<P>(rho); pw[2] = fe_mul(pw[1], pw[1]);
  Fe<P> acc[3] = {fe_zero<P>(), fe_zero<P>(), fe_zero<P>()};
  for (uint32_t k = lo + threadIdx.x; k < hi; k += 256) acc[0] = fe_add(acc[0], spmvt_entry<P>(rows, cm, dict, eq, pw, k));
  block_tree<P, 1>(acc, lds);
  if (threadIdx.x == 0) fe_store<P>(out + (size_t)c * 32, fe_load<P>(lds));
}

// a heavy column shared by SPMVT_PARTS workgroups (the constant column of the step circuit has ~3t entries: one
// workgroup walking them was 0.5 ms): each sums a contiguous chunk into a partial, k_spmvt_heavy_sum adds the partials
static constexpr uint32_t SPMVT_PARTS = 64;
template <class P>
__global__ __launch_bounds__(256) void k_spmvt_heavy_part(const uint32_t* __restrict__ heavy, const uint32_t* __restrict__ colptr,
                                                          const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cm,
                                                          const char* __restrict__ dict, const char* __restrict__ eq, FeArg rho,
                                                          char* __restrict__ partials) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[256 * 3 * 32];
  const uint32_t item = blockIdx.x / SPMVT_PARTS, part = blockIdx.x % SPMVT_PARTS;
  const uint32_t c = heavy[item];
  const uint32_t lo = colptr[c], hi = colptr[c + 1];
  const uint32_t chunk = (hi - lo + SPMVT_PARTS - 1) / SPMVT_PARTS;
  const uint32_t k0 = lo + part * chunk, k1 = (k0 + chunk < hi) ? k0 + chunk : hi;
  Fe<P> pw[3];
  pw[0] = fe_one<P>(); pw[1] = arg_fe<P>(rho); pw[2] = fe_mul(pw[1], pw[1]);
  Fe<P> acc[3] = {fe_zero<P>(), fe_zero<P>(), fe_zero<P>()};
  for (uint32_t k = k0 + threadIdx.x; k < k1; k += 256) acc[0] = fe_add(acc[0], spmvt_entry<P>(rows, cm, dict, eq, pw, k));
  block_tree<P, 1>(acc, lds);
  if (threadIdx.x == 0) fe_store<P>(partials + (size_t)blockIdx.x * 32, fe_load<P>(lds));
}
template <class P>
__global__ __launch_bounds__(64) void k_spmvt_heavy_sum(const uint32_t* __restrict__ heavy, const char* __restrict__ partials,
                                                        char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[64 * 32];
  fe_store<P>(lds + (size_t)threadIdx.x * 32, fe_load<P>(partials + ((size_t)blockIdx.x * SPMVT_PARTS + threadIdx.x) * 32));
  __syncthreads();
  for (int stride = 32; stride >= 1; stride >>= 1) {
    if ((int)threadIdx.x < stride) {
      char* p = lds + (size_t)threadIdx.x * 32;
      fe_store<P>(p, fe_add(fe_load<P>(p), fe_load<P>(p + (size_t)stride * 32)));
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) fe_store<P>(out + (size_t)heavy[blockIdx.x] * 32, fe_load<P>(lds));
}

// scratch: snark_reduce_scratch_bytes() bytes (the context's reduction scratch), or nullptr
Status snark_spmvt(int field, const uint32_t* colptr, const uint32_t* rows, const uint32_t* cm, const uint32_t* heavy,
                   size_t nheavy, size_t nbig, const void* dict, const void* eq, const vdf_fe* rho, size_t ncols, void* out,
                   void* scratch, hipStream_t s) {
  if (ncols == 0) return Status{};
  const FeArg r = to_arg(rho);
  VDF_TRY(with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_spmvt<tag_t<decltype(f)>>), grid_for(ncols), dim3(256), 0, s, colptr, rows, cm, cbytes_of(dict), cbytes_of(eq), r, ncols,
                       bytes_of(out));
  }));
  if (!nheavy) return Status{};
  // the list is sorted longest first: the first `nbig` columns (thousands of entries) are shared by SPMVT_PARTS workgroups
  // each, as far as the scratch reaches; the others get one workgroup each
  size_t shared = 0;
  if (scratch) {
    shared = nbig < nheavy ? nbig : nheavy;
    const size_t room = snark_reduce_scratch_bytes() / (SPMVT_PARTS * 32);
    if (shared > room) shared = room;
  }
  if (shared) {
    VDF_TRY(with_field(field, [&](auto f) {
      hipLaunchKernelGGL((k_spmvt_heavy_part<tag_t<decltype(f)>>), dim3((unsigned)(shared * SPMVT_PARTS)), dim3(256), 0, s, heavy, colptr, rows, cm,
                         cbytes_of(dict), cbytes_of(eq), r, bytes_of(scratch));
    }));
    VDF_TRY(with_field(field, [&](auto f) {
      hipLaunchKernelGGL((k_spmvt_heavy_sum<tag_t<decltype(f)>>), dim3((unsigned)shared), dim3(64), 0, s, heavy, cbytes_of(scratch), bytes_of(out));
    }));
  }
  if (nheavy > shared)
    return with_field(field, [&](auto f) {
      hipLaunchKernelGGL((k_spmvt_heavy<tag_t<decltype(f)>>), dim3((unsigned)(nheavy - shared)), dim3(256), 0, s, heavy + shared, colptr, rows, cm,
                         cbytes_of(dict), cbytes_of(eq), r, bytes_of(out));
    });
  return Status{};
}

// ---- inner-product argument helpers ------------------------------------------------------------------------
// Folded generators are never materialised: G^(j)_i = sum over the original indices t = i (mod n_j) of s[t] G_t, so a
// round's L = <a_lo, G_hi> and R = <a_hi, G_lo> are MSMs over the ORIGINAL generators with these scalars:
//   sL[t] = s[t] a[(t mod n_j) - h]  if (t mod n_j) >= h  else 0        sR[t] = s[t] a[(t mod n_j) + h]  if (t mod n_j) < h  else 0
template <class P>
__global__ __launch_bounds__(256) void k_ipa_scalars(const char* __restrict__ a, const char* __restrict__ sv, size_t n,
                                                     size_t nj, char* __restrict__ sL, char* __restrict__ sR) {
  __builtin_amdgcn_s_setprio(3);
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const size_t r = t & (nj - 1), h = nj >> 1;
  const Fe<P> sc = fe_load<P>(sv + t * 32);
  const Fe<P> z = fe_zero<P>();
  if (r >= h) {
    fe_store<P>(sL + t * 32, fe_mul(sc, fe_load<P>(a + (r - h) * 32)));
    fe_store<P>(sR + t * 32, z);
  } else {
    fe_store<P>(sL + t * 32, z);
    fe_store<P>(sR + t * 32, fe_mul(sc, fe_load<P>(a + (r + h) * 32)));
  }
}

template <class P>
__global__ __launch_bounds__(256) void k_scale_pattern(char* __restrict__ sv, size_t n, size_t nj, FeArg x_lo, FeArg x_hi) {
  __builtin_amdgcn_s_setprio(3);
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const bool upper = (t & (nj - 1)) >= (nj >> 1);
  fe_store<P>(sv + t * 32, fe_mul(fe_load<P>(sv + t * 32), arg_fe<P>(upper ? x_hi : x_lo)));
}

Status snark_ipa_scalars(int field, const void* a, const void* sv, size_t n, size_t nj, void* sL, void* sR, hipStream_t s) {
  if (n == 0 || (n & (n - 1)) || nj < 2 || (nj & (nj - 1)) || nj > n) return Status{VDF_ERR_BAD_LENGTH, "lengths must be powers of two, 2 <= n_j <= n"};
  KTimer kt(s, "k_ipa_scalars", 96.0 * n + 32.0 * nj);           // s read, sL and sR written, a read once
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_ipa_scalars<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, cbytes_of(a), cbytes_of(sv), n, nj, bytes_of(sL), bytes_of(sR));
  });
}

Status snark_scale_pattern(int field, void* sv, size_t n, size_t nj, const vdf_fe* x_lo, const vdf_fe* x_hi, hipStream_t s) {
  if (n == 0 || (n & (n - 1)) || nj < 2 || (nj & (nj - 1)) || nj > n) return Status{VDF_ERR_BAD_LENGTH, "lengths must be powers of two, 2 <= n_j <= n"};
  KTimer kt(s, "k_scale_pattern", 64.0 * n);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_scale_pattern<tag_t<decltype(f)>>), grid_for(n), dim3(256), 0, s, bytes_of(sv), n, nj, to_arg(x_lo), to_arg(x_hi));
  });
}

// ---- the same passes for many instances at once (vdf_reduce_batch, vdf_fold_halves_batch, vdf_spmv3_t_batch) ----------
// The instances' pointers and factors live in a device block (the context's argument block, one copy per call) read at
// wave-uniform addresses; an instance is blockIdx.y of the grid, so a round of K proofs is one launch of K times the rows.
struct ReduceItemDev { const char* t[5]; FeArg u; };
struct FoldItemDev { char* v; FeArg c_lo, c_hi; };
struct SpmvtItemDev { const char* eq; char* out; FeArg rho; };

size_t snark_reduce_item_bytes() { return sizeof(ReduceItemDev); }
size_t snark_fold_item_bytes() { return sizeof(FoldItemDev); }
size_t snark_spmvt_item_bytes() { return sizeof(SpmvtItemDev); }

void snark_reduce_pack(int kind, int count, const void* const tables[], const vdf_fe* u, void* block) {
  const int ntab = kind == 2 ? 5 : 2;
  ReduceItemDev* d = reinterpret_cast<ReduceItemDev*>(block);
  for (int q = 0; q < count; ++q) {
    ReduceItemDev it{};
    for (int k = 0; k < ntab; ++k) it.t[k] = cbytes_of(tables[(size_t)q * ntab + k]);
    if (u) it.u = to_arg(&u[q]);
    std::memcpy(&d[q], &it, sizeof(it));
  }
}

void snark_fold_pack(int k, void* const v[], const vdf_fe c_lo[], const vdf_fe c_hi[], void* block) {
  FoldItemDev* d = reinterpret_cast<FoldItemDev*>(block);
  for (int t = 0; t < k; ++t) {
    FoldItemDev it{};
    it.v = bytes_of(v[t]); it.c_lo = to_arg(&c_lo[t]); it.c_hi = to_arg(&c_hi[t]);
    std::memcpy(&d[t], &it, sizeof(it));
  }
}

void snark_spmvt_pack(int count, const void* const eq[], const vdf_fe rho[], void* const out[], void* block) {
  SpmvtItemDev* d = reinterpret_cast<SpmvtItemDev*>(block);
  for (int q = 0; q < count; ++q) {
    SpmvtItemDev it{};
    it.eq = cbytes_of(eq[q]); it.out = bytes_of(out[q]); it.rho = to_arg(&rho[q]);
    std::memcpy(&d[q], &it, sizeof(it));
  }
}

template <class P, int KIND>
__global__ __launch_bounds__(256) void k_reduce_batch(const ReduceItemDev* __restrict__ items, size_t n, char* __restrict__ partials) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[256 * 3 * 32];
  constexpr int NOUT = ReduceOuts<KIND>::N;
  const ReduceItemDev& it = items[blockIdx.y];
  ReduceArgs a;
#pragma unroll
  for (int k = 0; k < 5; ++k) a.t[k] = it.t[k];
  a.u = it.u;
  a.n = n;
  const size_t h = KIND == 0 ? n : n / 2;
  Fe<P> acc[3] = {fe_zero<P>(), fe_zero<P>(), fe_zero<P>()};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < h; i += (size_t)gridDim.x * 256) reduce_term<P, KIND>(a, i, h, acc);
  block_tree<P, NOUT>(acc, lds);
  const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (threadIdx.x < NOUT) fe_store<P>(partials + (slot * NOUT + threadIdx.x) * 32, fe_load<P>(lds + (size_t)threadIdx.x * 256 * 32));
}

// one workgroup per instance over that instance's nblocks partials
template <class P, int NOUT>
__global__ __launch_bounds__(256) void k_reduce_final_batch(const char* __restrict__ partials, int nblocks, char* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[256 * 3 * 32];
  const char* p = partials + (size_t)blockIdx.x * nblocks * NOUT * 32;
  Fe<P> acc[3] = {fe_zero<P>(), fe_zero<P>(), fe_zero<P>()};
  for (int b = threadIdx.x; b < nblocks; b += 256)
    for (int k = 0; k < NOUT; ++k) acc[k] = fe_add(acc[k], fe_load<P>(p + ((size_t)b * NOUT + k) * 32));
  block_tree<P, NOUT>(acc, lds);
  if (threadIdx.x < NOUT)
    fe_store<P>(out + ((size_t)blockIdx.x * NOUT + threadIdx.x) * 32, fe_load<P>(lds + (size_t)threadIdx.x * 256 * 32));
}

template <class P, int KIND>
static Status reduce_batch_launch(const void* block, int count, size_t n, void* scratch, void* out, hipStream_t s) {
  constexpr int NOUT = ReduceOuts<KIND>::N;
  const size_t h = KIND == 0 ? n : n / 2;
  // the grid spans instances x rows: REDUCE_BLOCKS workgroups shared among the instances (at least one each), so the
  // partials of a call fit the context's reduction scratch for count <= REDUCE_BLOCKS
  int per = REDUCE_BLOCKS / count;
  if (per < 1) per = 1;
  int need = (int)((h + 255) / 256);
  if (need < 1) need = 1;
  if (per > need) per = need;
  hipLaunchKernelGGL((k_reduce_batch<P, KIND>), dim3((unsigned)per, (unsigned)count), dim3(256), 0, s, reinterpret_cast<const ReduceItemDev*>(block), n,
                     bytes_of(scratch));
  hipLaunchKernelGGL((k_reduce_final_batch<P, NOUT>), dim3((unsigned)count), dim3(256), 0, s, cbytes_of(scratch), per, bytes_of(out));
  VDF_TRY_HIP(hipGetLastError());
  return Status{};
}

Status snark_reduce_batch(int field, int kind, const void* block, int count, size_t n, void* scratch, void* out, hipStream_t s) {
  if (kind < 0 || kind > 3) return Status{VDF_ERR_BAD_ARG, BAD_KIND};
  static_assert(SNARK_REDUCE_BATCH_MAX <= REDUCE_BLOCKS, "the partials of a batch fill the reduction scratch");
  if (count < 0 || count > SNARK_REDUCE_BATCH_MAX) return Status{VDF_ERR_BAD_ARG, "0..512 instances"};
  if (kind != 0 && (n < 2 || (n & (n - 1)))) return Status{VDF_ERR_BAD_LENGTH, "length must be a power of two >= 2"};
  if (count == 0) return Status{};
  KTimer kt(s, "k_reduce_batch", 32.0 * n * (kind == 2 ? 5 : 2) * count);
  return with_field(field, [&](auto f) {
    return with_int<0, 1, 2, 3>(kind, BAD_KIND, [&](auto k) {
      return reduce_batch_launch<tag_t<decltype(f)>, k.value>(block, count, n, scratch, out, s);
    });
  });
}

template <class P>
__global__ __launch_bounds__(256) void k_fold_halves_batch(const FoldItemDev* __restrict__ items, size_t h) {
  __builtin_amdgcn_s_setprio(3);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= h) return;
  const FoldItemDev& it = items[blockIdx.y];
  char* v = it.v;
  const Fe<P> lo = fe_load<P>(v + i * 32), hi = fe_load<P>(v + (h + i) * 32);
  fe_store<P>(v + i * 32, fe_add(fe_mul(arg_fe<P>(it.c_lo), lo), fe_mul(arg_fe<P>(it.c_hi), hi)));
}

Status snark_fold_halves_batch(int field, const void* block, int k, size_t n, hipStream_t s) {
  if (k <= 0) return Status{};
  if (k > SNARK_FOLD_BATCH_MAX) return Status{VDF_ERR_BAD_ARG, "at most 320 vectors"};
  if (n < 2 || (n & (n - 1))) return Status{VDF_ERR_BAD_LENGTH, "length must be a power of two >= 2"};
  const size_t h = n / 2;
  KTimer kt(s, "k_fold_halves_batch", 96.0 * h * k);
  return with_field(field, [&](auto f) {
    hipLaunchKernelGGL((k_fold_halves_batch<tag_t<decltype(f)>>), dim3((unsigned)((h + 255) / 256), (unsigned)k), dim3(256), 0, s,
                       reinterpret_cast<const FoldItemDev*>(block), h);
  });
}

// M-vectors of up to SPMVT_BATCH instances in one pass over the column structure: a column's pointers, rows and coefficient
// indices are read once, each lane carries one accumulator per instance (and the instance's rho, rho^2)
template <class P, int CB>
__device__ __forceinline__ void spmvt_entry_batch(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cm,
                                                  const char* __restrict__ dict, const SpmvtItemDev* __restrict__ items, int cnt,
                                                  const Fe<P> (&pw)[CB][2], uint32_t k, Fe<P> (&acc)[CB]) {
  const uint32_t c = cm[k], ci = c & 0x3FFFFFFFu, mat = c >> 30;
  const size_t row = rows[k];
  Fe<P> coef = fe_zero<P>();
  if (ci > 1) coef = fe_load<P>(dict + (size_t)ci * 32);
#pragma unroll
  for (int q = 0; q < CB; ++q) {
    if (q >= cnt) break;
    Fe<P> v = fe_load<P>(items[q].eq + row * 32);
    if (ci == 1) v = fe_neg(v);
    else if (ci > 1) v = fe_mul(v, coef);
    if (mat) v = fe_mul(v, pw[q][mat - 1]);
    acc[q] = fe_add(acc[q], v);
  }
}

template <class P, int CB>
__device__ __forceinline__ void spmvt_powers(const SpmvtItemDev* __restrict__ items, int cnt, Fe<P> (&pw)[CB][2]) {
#pragma unroll
  for (int q = 0; q < CB; ++q) {
    pw[q][0] = q < cnt ? arg_fe<P>(items[q].rho) : fe_zero<P>();
    pw[q][1] = fe_mul(pw[q][0], pw[q][0]);
  }
}

template <class P, int CB>
__global__ __launch_bounds__(256) void k_spmvt_batch(const uint32_t* __restrict__ colptr, const uint32_t* __restrict__ rows,
                                                     const uint32_t* __restrict__ cm, const char* __restrict__ dict,
                                                     const SpmvtItemDev* __restrict__ items, int cnt, size_t ncols) {
  __builtin_amdgcn_s_setprio(3);
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= ncols) return;
  const uint32_t lo = colptr[c], hi = colptr[c + 1];
  if (hi - lo > SPMVT_HEAVY) return;                            // the heavy kernels write this column
  Fe<P> pw[CB][2], acc[CB];
  spmvt_powers<P, CB>(items, cnt, pw);
#pragma unroll
  for (int q = 0; q < CB; ++q) acc[q] = fe_zero<P>();
  for (uint32_t k = lo; k < hi; ++k) spmvt_entry_batch<P, CB>(rows, cm, dict, items, cnt, pw, k, acc);
#pragma unroll
  for (int q = 0; q < CB; ++q)
    if (q < cnt) fe_store<P>(items[q].out + c * 32, acc[q]);
}

// heavy columns: a workgroup per column (part = 1) or SPMVT_PARTS workgroups per column, each over a contiguous chunk,
// into partials [column][part][instance] that k_spmvt_heavy_sum_batch adds
template <class P, int CB>
__global__ __launch_bounds__(256) void k_spmvt_heavy_batch(const uint32_t* __restrict__ heavy, const uint32_t* __restrict__ colptr,
                                                           const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cm,
                                                           const char* __restrict__ dict, const SpmvtItemDev* __restrict__ items,
                                                           int cnt, uint32_t parts, char* __restrict__ partials) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[256 * 32];
  const uint32_t item = blockIdx.x / parts, part = blockIdx.x % parts;
  const uint32_t c = heavy[item];
  const uint32_t lo = colptr[c], hi = colptr[c + 1];
  const uint32_t chunk = (hi - lo + parts - 1) / parts;
  const uint32_t k0 = lo + part * chunk, k1 = (k0 + chunk < hi) ? k0 + chunk : hi;
  Fe<P> pw[CB][2], acc[CB];
  spmvt_powers<P, CB>(items, cnt, pw);
#pragma unroll
  for (int q = 0; q < CB; ++q) acc[q] = fe_zero<P>();
  for (uint32_t k = k0 + threadIdx.x; k < k1; k += 256) spmvt_entry_batch<P, CB>(rows, cm, dict, items, cnt, pw, k, acc);
  for (int q = 0; q < cnt; ++q) {                               // one instance at a time through the LDS tree
    Fe<P> one_acc[3] = {acc[0], fe_zero<P>(), fe_zero<P>()};
#pragma unroll
    for (int j = 0; j < CB; ++j) if (j == q) one_acc[0] = acc[j];
    block_tree<P, 1>(one_acc, lds);
    if (threadIdx.x == 0) {
      if (parts == 1) fe_store<P>(items[q].out + (size_t)c * 32, fe_load<P>(lds));
      else fe_store<P>(partials + ((size_t)blockIdx.x * CB + q) * 32, fe_load<P>(lds));
    }
    __syncthreads();
  }
}

template <class P, int CB>
__global__ __launch_bounds__(64) void k_spmvt_heavy_sum_batch(const uint32_t* __restrict__ heavy, const char* __restrict__ partials,
                                                              const SpmvtItemDev* __restrict__ items) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ __align__(16) char lds[64 * 32];
  const int q = blockIdx.y;
  fe_store<P>(lds + (size_t)threadIdx.x * 32, fe_load<P>(partials + (((size_t)blockIdx.x * SPMVT_PARTS + threadIdx.x) * CB + q) * 32));
  __syncthreads();
  for (int stride = 32; stride >= 1; stride >>= 1) {
    if ((int)threadIdx.x < stride) {
      char* p = lds + (size_t)threadIdx.x * 32;
      fe_store<P>(p, fe_add(fe_load<P>(p), fe_load<P>(p + (size_t)stride * 32)));
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) fe_store<P>(items[q].out + (size_t)heavy[blockIdx.x] * 32, fe_load<P>(lds));
}

template <class P, int CB>
static Status spmvt_batch_launch(const uint32_t* colptr, const uint32_t* rows, const uint32_t* cm, const uint32_t* heavy,
                                 size_t nheavy, size_t nbig, const char* dict, const SpmvtItemDev* items, int cnt, size_t ncols,
                                 void* scratch, hipStream_t s) {
  hipLaunchKernelGGL((k_spmvt_batch<P, CB>), grid_for(ncols), dim3(256), 0, s, colptr, rows, cm, dict, items, cnt, ncols);
  if (nheavy) {
    // as snark_spmvt: the longest columns shared by SPMVT_PARTS workgroups each, as far as the scratch holds their partials
    size_t shared = nbig < nheavy ? nbig : nheavy;
    const size_t room = snark_reduce_scratch_bytes() / ((size_t)SPMVT_PARTS * CB * 32);
    if (shared > room) shared = room;
    char* part = bytes_of(scratch);
    if (shared) {
      hipLaunchKernelGGL((k_spmvt_heavy_batch<P, CB>), dim3((unsigned)(shared * SPMVT_PARTS)), dim3(256), 0, s, heavy, colptr, rows,
                         cm, dict, items, cnt, SPMVT_PARTS, part);
      hipLaunchKernelGGL((k_spmvt_heavy_sum_batch<P, CB>), dim3((unsigned)shared, (unsigned)cnt), dim3(64), 0, s, heavy, cbytes_of(part), items);
    }
    if (nheavy > shared)
      hipLaunchKernelGGL((k_spmvt_heavy_batch<P, CB>), dim3((unsigned)(nheavy - shared)), dim3(256), 0, s, heavy + shared, colptr,
                         rows, cm, dict, items, cnt, 1u, part);
  }
  VDF_TRY_HIP(hipGetLastError());
  return Status{};
}

// block: count SpmvtItemDev; launches of up to SPMVT_BATCH instances each, one after the other on the stream (the heavy
// columns' partials reuse the scratch)
Status snark_spmvt_batch(int field, const uint32_t* colptr, const uint32_t* rows, const uint32_t* cm, const uint32_t* heavy,
                         size_t nheavy, size_t nbig, const void* dict, const void* block, int count, size_t ncols, void* scratch,
                         hipStream_t s) {
  if (ncols == 0 || count <= 0) return Status{};
  const SpmvtItemDev* items = reinterpret_cast<const SpmvtItemDev*>(block);
  return with_field(field, [&](auto f) {
    for (int q0 = 0; q0 < count; q0 += SPMVT_BATCH) {
      const int cnt = count - q0 < SPMVT_BATCH ? count - q0 : SPMVT_BATCH;
      // the kernel's width: 1, 2, or SPMVT_BATCH accumulators per lane (3 instances run in the widest)
      VDF_TRY((with_int<1, 2, SPMVT_BATCH>(cnt <= 2 ? cnt : SPMVT_BATCH, "batch width", [&](auto cb) {
        return spmvt_batch_launch<tag_t<decltype(f)>, cb.value>(colptr, rows, cm, heavy, nheavy, nbig, cbytes_of(dict), items + q0, cnt, ncols,
                                                               scratch, s);
      })));
    }
    return Status{};
  });
}

}  // namespace vdf
