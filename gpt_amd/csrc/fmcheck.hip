// Test entries for the noise path (gpt_debug_fastmath, gpt_debug_normals; include/gptsgld.h): the
// inline functions of fastmath.h and gpt_common.h evaluated on given inputs, called exactly as the
// engines call them — the coefficient table through fm_coef(), the two 16-entry sin/cos tables
// filled in LDS by sincos_tab_fill — and compiled with the flags of the engines.  Nothing is
// restated here; tests/test_gpu_fastmath.py holds the results to mpmath.
#include "host_util.h"

namespace gpt {

constexpr int kFmNT = 256;

enum FmFn : int {
  kFmLog = 0, kFmSqrt = 1, kFmRcp = 2, kFmSincos = 3, kFmSincosTab2 = 4, kFmTable = 5, kFmU53 = 6,
  kFmU32 = 7, kFmRadius = 8, kFmCount = 9
};
enum NormGen : int {
  kGenAt = 0, kGenPair = 1, kGenQuad4 = 2, kGenQuad2 = 3, kGenQuadTab4 = 4, kGenQuadTab2 = 5,
  kGenHost = 6, kGenCount = 7
};

template <int FN>
__global__ __launch_bounds__(kFmNT) void fm_check_kernel(long long count, const double* x,
                                                         const uint32_t* xi, double* out0,
                                                         double* out1) {
  __shared__ __attribute__((aligned(16))) double tab[64];
  if constexpr (FN == kFmSincosTab2 || FN == kFmTable) {
    sincos_tab_fill(tab, (int)threadIdx.x, kFmNT);
    __syncthreads();
  }
  const long long i = (long long)blockIdx.x * kFmNT + threadIdx.x;
  if (i >= count) return;
  const auto c = fm_coef();
  (void)c;
  if constexpr (FN == kFmLog) out0[i] = fm_log_c(x[i], c);
  if constexpr (FN == kFmSqrt) out0[i] = fm_sqrt_pos(x[i]);
  if constexpr (FN == kFmRcp) out0[i] = fm_rcp(x[i]);
  if constexpr (FN == kFmRadius) out0[i] = fm_sqrt_pos(-2.0 * fm_log_c(x[i], c));
  if constexpr (FN == kFmSincos) {
    double sn, cs;
    fm_sincos_2pi_c(x[i], sn, cs, c);
    out0[i] = sn;
    out1[i] = cs;
  }
  if constexpr (FN == kFmSincosTab2) {
    double sn, cs;
    fm_sincos_tab2(xi[i], tab, sn, cs, c);
    out0[i] = sn;
    out1[i] = cs;
  }
  if constexpr (FN == kFmTable) out0[i] = tab[i];
  if constexpr (FN == kFmU53) out0[i] = u53(xi[2 * i], xi[2 * i + 1]);
  if constexpr (FN == kFmU32) out0[i] = u32u(xi[i]);
}

// Block b of the launch is Philox block c0 = c0_first + b: its four words, and the 2 or 4 normals
// generator GEN makes of it.
template <int GEN>
__global__ __launch_bounds__(kFmNT) void normals_check_kernel(uint64_t seed, uint32_t c0_first,
                                                              long long nblocks, uint32_t c1,
                                                              uint32_t c2, uint32_t c3, double* z,
                                                              uint32_t* words) {
  __shared__ __attribute__((aligned(16))) double tab[64];
  if constexpr (GEN == kGenQuadTab4 || GEN == kGenQuadTab2) {
    sincos_tab_fill(tab, (int)threadIdx.x, kFmNT);
    __syncthreads();
  }
  const long long b = (long long)blockIdx.x * kFmNT + threadIdx.x;
  if (b >= nblocks) return;
  const uint32_t c0 = c0_first + (uint32_t)b;
  const U4 w = philox4x32(c0, c1, c2, c3, seed);
  words[4 * b] = w.x;
  words[4 * b + 1] = w.y;
  words[4 * b + 2] = w.z;
  words[4 * b + 3] = w.w;
  if constexpr (GEN == kGenAt) {
    z[2 * b] = normal_at(seed, 2u * c0, c1, c2, c3);
    z[2 * b + 1] = normal_at(seed, 2u * c0 + 1u, c1, c2, c3);
  }
  if constexpr (GEN == kGenPair) normal_pair(seed, c0, c1, c2, c3, z[2 * b], z[2 * b + 1]);
  if constexpr (GEN == kGenQuad4) normal_quad<4>(seed, c0, c1, c2, c3, z + 4 * b);
  if constexpr (GEN == kGenQuad2) normal_quad<2>(seed, c0, c1, c2, c3, z + 2 * b);
  if constexpr (GEN == kGenQuadTab4) normal_quad_tab<4>(seed, c0, c1, c2, c3, tab, z + 4 * b);
  if constexpr (GEN == kGenQuadTab2) normal_quad_tab<2>(seed, c0, c1, c2, c3, tab, z + 2 * b);
}

namespace {

template <int FN>
void fm_launch(long long count, const double* x, const uint32_t* xi, double* o0, double* o1) {
  hipLaunchKernelGGL(fm_check_kernel<FN>, dim3((unsigned)((count + kFmNT - 1) / kFmNT)),
                     dim3(kFmNT), 0, nullptr, count, x, xi, o0, o1);
}
template <int GEN>
void normals_launch(uint64_t seed, uint32_t c0_first, long long nblocks, uint32_t c1, uint32_t c2,
                    uint32_t c3, double* z, uint32_t* words) {
  hipLaunchKernelGGL(normals_check_kernel<GEN>, dim3((unsigned)((nblocks + kFmNT - 1) / kFmNT)),
                     dim3(kFmNT), 0, nullptr, seed, c0_first, nblocks, c1, c2, c3, z, words);
}

constexpr long long kFmMaxCount = 1ll << 24;   // elements / Philox blocks per call

}  // namespace
}  // namespace gpt

using namespace gpt;

extern "C" int gpt_debug_fastmath(int32_t fn, int64_t count, const double* x, const uint32_t* xi,
                                  double* out0, double* out1) {
  if (fn < 0 || fn >= kFmCount) { set_error("gpt_debug_fastmath: unknown fn"); return GPT_ERR_BAD_DIMS; }
  const bool words = fn == kFmSincosTab2 || fn == kFmU53 || fn == kFmU32;
  const bool two = fn == kFmSincos || fn == kFmSincosTab2;
  const bool ok = count >= 1 && count <= kFmMaxCount && out0 && (!two || out1) &&
                  (fn == kFmTable ? count == 64 : (words ? xi != nullptr : x != nullptr));
  if (!ok) { set_error("gpt_debug_fastmath: bad arguments"); return GPT_ERR_BAD_DIMS; }
  DevMem din, d0, d1;
  if (fn == kFmTable) GPT_HIPCHK(din.alloc<double>(0));
  else if (words) GPT_HIPCHK(din.upload(xi, (size_t)count * (fn == kFmU53 ? 2 : 1)));
  else GPT_HIPCHK(din.upload(x, (size_t)count));
  GPT_HIPCHK(d0.alloc<double>(count));
  GPT_HIPCHK(d1.alloc<double>(count));
  const double* dx = din.as<double>();
  const uint32_t* dxi = din.as<uint32_t>();
  double *o0 = d0.as<double>(), *o1 = d1.as<double>();
  switch (fn) {
    case kFmLog: fm_launch<kFmLog>(count, dx, dxi, o0, o1); break;
    case kFmSqrt: fm_launch<kFmSqrt>(count, dx, dxi, o0, o1); break;
    case kFmRcp: fm_launch<kFmRcp>(count, dx, dxi, o0, o1); break;
    case kFmSincos: fm_launch<kFmSincos>(count, dx, dxi, o0, o1); break;
    case kFmSincosTab2: fm_launch<kFmSincosTab2>(count, dx, dxi, o0, o1); break;
    case kFmTable: fm_launch<kFmTable>(count, dx, dxi, o0, o1); break;
    case kFmU53: fm_launch<kFmU53>(count, dx, dxi, o0, o1); break;
    case kFmU32: fm_launch<kFmU32>(count, dx, dxi, o0, o1); break;
    default: fm_launch<kFmRadius>(count, dx, dxi, o0, o1); break;
  }
  GPT_HIPCHK(hipGetLastError());
  GPT_HIPCHK(hipDeviceSynchronize());
  GPT_HIPCHK(d0.download(out0, count));
  if (two) GPT_HIPCHK(d1.download(out1, count));
  return GPT_OK;
}

extern "C" int gpt_debug_normals(int32_t gen, uint64_t seed, uint32_t c0_first, int64_t nblocks,
                                 uint32_t c1, uint32_t c2, uint32_t c3, double* z,
                                 uint32_t* words) {
  if (gen < 0 || gen >= kGenCount) { set_error("gpt_debug_normals: unknown gen"); return GPT_ERR_BAD_DIMS; }
  // normal_at's element index 2·c0 + 1 is a 32-bit word: its last block is c0 = 2^31 − 1
  const long long top = gen == kGenAt ? 1ll << 31 : 1ll << 32;
  if (nblocks < 1 || nblocks > kFmMaxCount || (long long)c0_first + nblocks > top || !z || !words) {
    set_error("gpt_debug_normals: bad arguments");
    return GPT_ERR_BAD_DIMS;
  }
  if (gen == kGenHost) {      // the host C++ philox4x32 and u53 (no device work)
    for (long long b = 0; b < nblocks; ++b) {
      const U4 w = philox4x32(c0_first + (uint32_t)b, c1, c2, c3, seed);
      words[4 * b] = w.x;
      words[4 * b + 1] = w.y;
      words[4 * b + 2] = w.z;
      words[4 * b + 3] = w.w;
      z[2 * b] = u53(w.x, w.y);
      z[2 * b + 1] = u53(w.z, w.w);
    }
    return GPT_OK;
  }
  const size_t per = (gen == kGenQuad4 || gen == kGenQuadTab4) ? 4 : 2;
  DevMem dz, dw;
  GPT_HIPCHK(dz.alloc<double>(per * (size_t)nblocks));
  GPT_HIPCHK(dw.alloc<uint32_t>(4 * (size_t)nblocks));
  double* pz = dz.as<double>();
  uint32_t* pw = dw.as<uint32_t>();
  switch (gen) {
    case kGenAt: normals_launch<kGenAt>(seed, c0_first, nblocks, c1, c2, c3, pz, pw); break;
    case kGenPair: normals_launch<kGenPair>(seed, c0_first, nblocks, c1, c2, c3, pz, pw); break;
    case kGenQuad4: normals_launch<kGenQuad4>(seed, c0_first, nblocks, c1, c2, c3, pz, pw); break;
    case kGenQuad2: normals_launch<kGenQuad2>(seed, c0_first, nblocks, c1, c2, c3, pz, pw); break;
    case kGenQuadTab4: normals_launch<kGenQuadTab4>(seed, c0_first, nblocks, c1, c2, c3, pz, pw); break;
    default: normals_launch<kGenQuadTab2>(seed, c0_first, nblocks, c1, c2, c3, pz, pw); break;
  }
  GPT_HIPCHK(hipGetLastError());
  GPT_HIPCHK(hipDeviceSynchronize());
  GPT_HIPCHK(dz.download(z, per * (size_t)nblocks));
  GPT_HIPCHK(dw.download(words, 4 * (size_t)nblocks));
  return GPT_OK;
}
