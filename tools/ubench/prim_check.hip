// Diagnostic (not product code): a data-driven runner for the field and curve primitives of fe.cuh, ec.cuh and ecq.cuh, in
// both fields.  It applies an operation to operands read from a job file, one lane per case (one quad per case for the QPoint
// operations), and writes the raw results; it compares NOTHING -- the reference is tests/prim_spec.py, in Python integers.
//
//   prim_check [--host] <jobs> <results>
//
// jobs:    "PRIMJOB1", u32 njobs, then per job  u32 field (0 Fp, 1 Fq), u32 op, u32 ncases, u32 nin,  ncases * nin words
// results: "PRIMOUT1", u32 njobs, then per job  u32 field, u32 op, u32 ncases, u32 nout,             ncases * nout words
// A word is 32 bytes, little endian; flags and small integers travel in the low limb of a word of their own.
// --host runs the same jobs through the host instantiation of the same headers (no HIP call at all); the operations that
// exist only on the device (xyzz_add_lazy, ecq.cuh) are refused there.  A HIP error or a malformed file: non-zero exit.
// Build: vdf_amd/csrc/Makefile (hipcc -O3 -std=c++17 --offload-arch=gfx950 -I vdf_amd/csrc).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fe.cuh"
#include "ec.cuh"
#include "ecq.cuh"
using namespace vdf;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)

// op, words in, words out, runs on the host, one quad per case
#define PRIM_OPS(X) \
  X(1, 2, 1, 1, 0)  /* fe_mul_lazy */      X(2, 1, 1, 1, 0)  /* fe_sqr_lazy */     X(3, 2, 1, 1, 0)  /* fe_mul_inl */ \
  X(4, 1, 1, 1, 0)  /* fe_sqr_inl */       X(5, 4, 1, 1, 0)  /* fe_mul2_lazy */    X(6, 2, 1, 1, 0)  /* fe_sub_lazy */ \
  X(7, 1, 1, 1, 0)  /* fe_neg_lazy */      X(8, 1, 1, 1, 0)  /* fe_neg_nz */       X(9, 1, 1, 1, 0)  /* fe_canon */ \
  X(10, 2, 1, 1, 0) /* fe_add */           X(11, 2, 1, 1, 0) /* fe_sub */          X(12, 1, 1, 1, 0) /* fe_neg */ \
  X(13, 1, 1, 1, 0) /* fe_dbl */           X(14, 1, 1, 1, 0) /* fe_from_small */   X(15, 1, 1, 1, 0) /* fe_from_mont */ \
  X(16, 1, 1, 1, 0) /* fe_to_mont */       X(17, 1, 1, 1, 0) /* fe_inv */          X(18, 1, 1, 1, 0) /* fe_is_canonical */ \
  X(19, 2, 1, 1, 0) /* fe_mul (the out-of-line call) */ \
  X(20, 8, 10, 1, 0)  /* xyzz_madd_lazy: acc, have, flip, b -> acc, have, flip, xyzz_lazy_resolve */ \
  X(21, 10, 10, 0, 0) /* xyzz_add_lazy:  acc, have, flip, b -> the same */ \
  X(22, 6, 4, 1, 0) /* xyzz_madd<false> */ X(23, 6, 4, 1, 0) /* xyzz_madd<true> */ X(24, 8, 4, 1, 0) /* xyzz_add */ \
  X(25, 4, 4, 1, 0) /* xyzz_dbl */         X(26, 2, 4, 1, 0) /* xyzz_dbl_affine */ X(27, 4, 3, 1, 0) /* xyzz_to_jac */ \
  X(28, 3, 4, 1, 0) /* jac_to_xyzz */      X(29, 4, 2, 1, 0) /* xyzz_to_affine */  X(30, 3, 4, 1, 0) /* xyzz_mul_u64: point, k */ \
  X(31, 2, 1, 1, 0) /* fe_mul_lazy_t31 */  X(32, 1, 1, 1, 0) /* fe_sqr_lazy_t31 */ X(33, 4, 1, 1, 0) /* fe_mul2_lazy_t31: limb 7 of every operand <= 0x80000000 */ \
  X(40, 8, 5, 0, 1) /* qpoint_add -> point, inf */   X(41, 4, 5, 0, 1) /* qpoint_dbl */   X(42, 4, 5, 0, 1) /* qpoint_neg */ \
  X(43, 4, 5, 0, 1) /* qpoint_load_lazy -> qpoint_store */ \
  X(44, 4, 5, 0, 1) /* qpoint_wave_sum over each 16 consecutive cases (ncases a multiple of 16) */

template <class P> VDF_HD Fe<P> word(uint32_t x) { Fe<P> r = fe_zero<P>(); r.v[0] = x; return r; }
template <class P> VDF_HD Fe<P> ld(const uint32_t* in, int k) { return fe_load<P>(in + 8 * k); }
template <class P> VDF_HD void st(uint32_t* out, int k, const Fe<P>& a) { fe_store<P>(out + 8 * k, a); }
template <class P> VDF_HD XYZZ<P> ld4(const uint32_t* in, int k) { return xyzz_load<P>(in + 8 * k); }
template <class P> VDF_HD void st4(uint32_t* out, int k, const XYZZ<P>& a) { xyzz_store<P>(out + 8 * k, a); }

// one case of a lane operation: `in` and `out` point at this case's words
template <class P, int OP> VDF_HD void apply(const uint32_t* in, uint32_t* out) {
  if constexpr (OP == 1) st<P>(out, 0, fe_mul_lazy(ld<P>(in, 0), ld<P>(in, 1)));
  else if constexpr (OP == 2) st<P>(out, 0, fe_sqr_lazy(ld<P>(in, 0)));
  else if constexpr (OP == 3) st<P>(out, 0, fe_mul_inl(ld<P>(in, 0), ld<P>(in, 1)));
  else if constexpr (OP == 4) st<P>(out, 0, fe_sqr_inl(ld<P>(in, 0)));
  else if constexpr (OP == 5) st<P>(out, 0, fe_mul2_lazy(ld<P>(in, 0), ld<P>(in, 1), ld<P>(in, 2), ld<P>(in, 3)));
  else if constexpr (OP == 6) st<P>(out, 0, fe_sub_lazy(ld<P>(in, 0), ld<P>(in, 1)));
  else if constexpr (OP == 7) st<P>(out, 0, fe_neg_lazy(ld<P>(in, 0)));
  else if constexpr (OP == 8) st<P>(out, 0, fe_neg_nz(ld<P>(in, 0)));
  else if constexpr (OP == 9) st<P>(out, 0, fe_canon(ld<P>(in, 0)));
  else if constexpr (OP == 10) st<P>(out, 0, fe_add(ld<P>(in, 0), ld<P>(in, 1)));
  else if constexpr (OP == 11) st<P>(out, 0, fe_sub(ld<P>(in, 0), ld<P>(in, 1)));
  else if constexpr (OP == 12) st<P>(out, 0, fe_neg(ld<P>(in, 0)));
  else if constexpr (OP == 13) st<P>(out, 0, fe_dbl(ld<P>(in, 0)));
  else if constexpr (OP == 14) st<P>(out, 0, fe_from_small<P>(in[0]));
  else if constexpr (OP == 15) st<P>(out, 0, fe_from_mont(ld<P>(in, 0)));
  else if constexpr (OP == 16) st<P>(out, 0, fe_to_mont(ld<P>(in, 0)));
  else if constexpr (OP == 17) st<P>(out, 0, fe_inv(ld<P>(in, 0)));
  else if constexpr (OP == 18) st<P>(out, 0, word<P>(fe_is_canonical(ld<P>(in, 0)) ? 1u : 0u));
  else if constexpr (OP == 19) st<P>(out, 0, fe_mul(ld<P>(in, 0), ld<P>(in, 1)));
  else if constexpr (OP == 20) {
    XYZZ<P> acc = ld4<P>(in, 0);
    bool have = in[8 * 4] != 0, flip = in[8 * 5] != 0;
    xyzz_madd_lazy<P>(acc, have, flip, affine_load<P>(in + 8 * 6));
    st4<P>(out, 0, acc); st<P>(out, 4, word<P>(have)); st<P>(out, 5, word<P>(flip));
    st4<P>(out, 6, xyzz_lazy_resolve<P>(acc, have, flip));
  } else if constexpr (OP == 21) {
#if defined(__HIP_DEVICE_COMPILE__)
    XYZZ<P> acc = ld4<P>(in, 0);
    bool have = in[8 * 4] != 0, flip = in[8 * 5] != 0;
    xyzz_add_lazy<P>(acc, have, flip, ld4<P>(in, 6));
    st4<P>(out, 0, acc); st<P>(out, 4, word<P>(have)); st<P>(out, 5, word<P>(flip));
    st4<P>(out, 6, xyzz_lazy_resolve<P>(acc, have, flip));
#endif
  } else if constexpr (OP == 22 || OP == 23) {
    XYZZ<P> acc = ld4<P>(in, 0);
    xyzz_madd<P, OP == 23>(acc, affine_load<P>(in + 8 * 4));
    st4<P>(out, 0, acc);
  } else if constexpr (OP == 24) {
    XYZZ<P> acc = ld4<P>(in, 0);
    xyzz_add(acc, ld4<P>(in, 4));
    st4<P>(out, 0, acc);
  } else if constexpr (OP == 25) st4<P>(out, 0, xyzz_dbl(ld4<P>(in, 0)));
  else if constexpr (OP == 26) st4<P>(out, 0, xyzz_dbl_affine(affine_load<P>(in)));
  else if constexpr (OP == 27) {
    const Jac<P> j = xyzz_to_jac(ld4<P>(in, 0));
    st<P>(out, 0, j.x); st<P>(out, 1, j.y); st<P>(out, 2, j.z);
  } else if constexpr (OP == 28) {
    Jac<P> j; j.x = ld<P>(in, 0); j.y = ld<P>(in, 1); j.z = ld<P>(in, 2);
    st4<P>(out, 0, jac_to_xyzz(j));
  } else if constexpr (OP == 29) affine_store<P>(out, xyzz_to_affine(ld4<P>(in, 0)));
  else if constexpr (OP == 30) st4<P>(out, 0, xyzz_mul_u64(affine_load<P>(in), (uint64_t)in[16] | ((uint64_t)in[17] << 32)));
  else if constexpr (OP == 31) st<P>(out, 0, fe_mul_lazy_t31(ld<P>(in, 0), ld<P>(in, 1)));
  else if constexpr (OP == 32) st<P>(out, 0, fe_sqr_lazy_t31(ld<P>(in, 0)));
  else if constexpr (OP == 33) st<P>(out, 0, fe_mul2_lazy_t31(ld<P>(in, 0), ld<P>(in, 1), ld<P>(in, 2), ld<P>(in, 3)));
}

template <class P, int OP> __global__ __launch_bounds__(64) void k_lane(const uint32_t* in, uint32_t* out, int n, int nin, int nout) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  apply<P, OP>(in + (size_t)i * nin * 8, out + (size_t)i * nout * 8);
}

// one quad per case; lane q of the quad touches coordinate q.  The early exit is quad-uniform (a case is a whole quad).
template <class P, int OP> __global__ __launch_bounds__(64) void k_quad(const char* in, char* out, int n, int nin, int nout) {
  const int i = (blockIdx.x * 64 + threadIdx.x) >> 2;
  if (i >= n) return;
  const char* ci = in + (size_t)i * nin * 32;
  char* co = out + (size_t)i * nout * 32;
  QPoint<P> r;
  if constexpr (OP == 40) r = qpoint_add<P>(qpoint_load<P>(ci), qpoint_load<P>(ci + 128));
  else if constexpr (OP == 41) r = qpoint_dbl<P>(qpoint_load<P>(ci));
  else if constexpr (OP == 42) r = qpoint_neg<P>(qpoint_load<P>(ci));
  else if constexpr (OP == 43) r = qpoint_load_lazy<P>(ci);
  else r = qpoint_wave_sum<P>(qpoint_load<P>(ci));
  qpoint_store<P>(co, r);
  if (quad_pos() == 0) fe_store<P>(co + 128, word<P>(r.inf ? 1u : 0u));
}

struct Job { uint32_t field, op, n, nin, nout; const uint32_t* in; std::vector<uint32_t> out; };

template <class P, int OP, bool HOST_OK, bool QUAD> int run(Job& j, bool host) {
  if (host) {
    if constexpr (HOST_OK) {
      for (uint32_t i = 0; i < j.n; ++i) apply<P, OP>(j.in + (size_t)i * j.nin * 8, j.out.data() + (size_t)i * j.nout * 8);
      return 0;
    } else {
      fprintf(stderr, "op %u exists only on the device\n", j.op);
      return 2;
    }
  }
  if (j.n == 0) return 0;
  const size_t bi = (size_t)j.n * j.nin * 32, bo = (size_t)j.n * j.nout * 32;
  uint32_t *din = nullptr, *dout = nullptr;
  CK(hipMalloc(&din, bi)); CK(hipMalloc(&dout, bo));
  CK(hipMemcpy(din, j.in, bi, hipMemcpyHostToDevice));
  CK(hipMemset(dout, 0xEE, bo));
  if constexpr (QUAD) {
    if (OP == 44 && j.n % 16) { fprintf(stderr, "qpoint_wave_sum needs whole wavefronts (16 cases each)\n"); return 2; }
    hipLaunchKernelGGL((k_quad<P, OP>), dim3((j.n * 4 + 63) / 64), dim3(64), 0, 0, (const char*)din, (char*)dout, (int)j.n, (int)j.nin, (int)j.nout);
  } else {
    hipLaunchKernelGGL((k_lane<P, OP>), dim3((j.n + 63) / 64), dim3(64), 0, 0, din, dout, (int)j.n, (int)j.nin, (int)j.nout);
  }
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(j.out.data(), dout, bo, hipMemcpyDeviceToHost));
  CK(hipFree(din)); CK(hipFree(dout));
  return 0;
}

static int dispatch(Job& j, bool host) {
  switch (j.op) {
#define X(OP, NIN, NOUT, HOST, QUAD) case OP: return j.field == 0 ? run<FpParams, OP, HOST, QUAD>(j, host) : run<FqParams, OP, HOST, QUAD>(j, host);
    PRIM_OPS(X)
#undef X
  }
  return 2;
}
static bool op_shape(uint32_t op, uint32_t& nin, uint32_t& nout) {
  switch (op) {
#define X(OP, NIN, NOUT, HOST, QUAD) case OP: nin = NIN; nout = NOUT; return true;
    PRIM_OPS(X)
#undef X
  }
  return false;
}

int main(int argc, char** argv) {
  bool host = false;
  int a = 1;
  if (a < argc && !strcmp(argv[a], "--host")) { host = true; ++a; }
  if (argc - a != 2) { fprintf(stderr, "usage: prim_check [--host] <jobs> <results>\n"); return 2; }
  FILE* f = fopen(argv[a], "rb");
  if (!f) { perror(argv[a]); return 2; }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<unsigned char> raw((size_t)(size > 0 ? size : 0));
  if (size < 12 || fread(raw.data(), 1, (size_t)size, f) != (size_t)size || memcmp(raw.data(), "PRIMJOB1", 8)) { fprintf(stderr, "not a job file\n"); return 2; }
  fclose(f);
  uint32_t njobs;
  memcpy(&njobs, raw.data() + 8, 4);
  size_t pos = 12;
  std::vector<Job> jobs;
  std::vector<std::vector<uint32_t>> operands;
  for (uint32_t k = 0; k < njobs; ++k) {
    if (pos + 16 > raw.size()) { fprintf(stderr, "truncated job header\n"); return 2; }
    uint32_t h[4];
    memcpy(h, raw.data() + pos, 16);
    pos += 16;
    Job j{};
    j.field = h[0]; j.op = h[1]; j.n = h[2]; j.nin = h[3];
    uint32_t nin = 0;
    if (j.field > 1 || !op_shape(j.op, nin, j.nout) || nin != j.nin || j.n > (1u << 20)) { fprintf(stderr, "job %u: bad field, op or shape\n", k); return 2; }
    const size_t bytes = (size_t)j.n * j.nin * 32;
    if (pos + bytes > raw.size()) { fprintf(stderr, "job %u: truncated operands\n", k); return 2; }
    operands.emplace_back(bytes / 4 + 8);
    memcpy(operands.back().data(), raw.data() + pos, bytes);
    pos += bytes;
    j.out.assign((size_t)j.n * j.nout * 8, 0u);
    jobs.push_back(std::move(j));
  }
  for (size_t k = 0; k < jobs.size(); ++k) {
    jobs[k].in = operands[k].data();
    const int rc = dispatch(jobs[k], host);
    if (rc) return rc;
  }
  FILE* g = fopen(argv[a + 1], "wb");
  if (!g) { perror(argv[a + 1]); return 2; }
  fwrite("PRIMOUT1", 1, 8, g);
  fwrite(&njobs, 4, 1, g);
  for (const Job& j : jobs) {
    const uint32_t h[4] = {j.field, j.op, j.n, j.nout};
    fwrite(h, 4, 4, g);
    fwrite(j.out.data(), 4, j.out.size(), g);
  }
  if (fclose(g)) { perror(argv[a + 1]); return 2; }
  printf("prim_check: %u jobs on the %s\n", njobs, host ? "host" : "device");
  return 0;
}
