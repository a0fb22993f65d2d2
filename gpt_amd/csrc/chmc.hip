// Hamiltonian Monte Carlo on the resident θ of the softmax classifier's joint likelihood for
// MI355X (gfx950): momentum, the leapfrog integrator, the Hamiltonian and the Metropolis decision
// around cjoint_eval_kernel<·, kCjTheta>, which stays the one evaluation of U = −log p(y, θ; h)
// and its θ partials.  DESIGN §6i.
//
// With s = √eps, one transition from θ is p ~ N(0, I); p ← p − ½s∇U(θ), q ← θ + s·p; L − 1 times
// p ← p − s∇U(q), q ← q + s·p; p ← p − ½s∇U(q); accept q iff u < exp(H0 − H1),
// H = U + ½‖p‖² (L = 1: the MALA loop of BloodTransfusionExperiment.jl:255-278).
//
// All fp64.  An entry of θ, q, p and of the reduced gradients has one owner thread, entry
// e = c·n + j owned by thread e of a grid of kNT-thread workgroups; ‖p‖² and ‖q‖² leave a
// workgroup as one partial (blk_sum's fixed pattern) and the partials are added in workgroup
// order by one thread, so every sum's order depends on the shape alone and there is no atomic on
// a double.  The potential of a state is formed by one function (hmc_potential) from the
// evaluation's value partials and the ‖·‖² partials, and its reduced gradient by one expression
// (hmc_grad), whether the state is the start of a run or a proposal: the cached U(θ) and ∇U(θ)
// of an accepted proposal are the bits a fresh evaluation at that θ gives.
#include <cfloat>

#include "device_util.h"

namespace gpt {

static __device__ __forceinline__ bool hmc_stopped(const int32_t* status) {
  return status && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// ∇U at the position x of the last evaluation: Σ_b part_theta[b][e] + x[e], the sum in workgroup
// order as cjoint_update_kernel forms it.
static __device__ __forceinline__ double hmc_grad(const double* __restrict__ part_theta, int nblk,
                                                  size_t nC, size_t e, double x) {
  double g = 0.0;
  for (int b = 0; b < nblk; ++b) g += part_theta[(size_t)b * nC + e];
  return g + x;
}

// Momentum of transition t and θ → q; kin0[workgroup] = Σ p² of its entries.  DRAW: p[j, c] is
// element j of the normal stream (seed, t, kHmcMom, c); otherwise p is the caller's.
template <bool DRAW>
__global__ __launch_bounds__(kNT) void hmc_begin_kernel(const HmcDev S, uint64_t seed, uint32_t t) {
  __shared__ double red[kNW];
  if (hmc_stopped(S.status)) return;
  const size_t nC = (size_t)S.n * S.C;
  const size_t e = (size_t)blockIdx.x * kNT + threadIdx.x;
  double p = 0.0;
  if (e < nC) {
    if constexpr (DRAW) {
      const int c = (int)(e / S.n), j = (int)(e - (size_t)c * S.n);
      p = normal_at(seed, (uint32_t)j, t, kHmcMom, (uint32_t)c);
      S.p[e] = p;
    } else {
      p = S.p[e];
    }
    S.q[e] = S.theta[e];
  }
  const double k = blk_sum(__dmul_rn(p, p), red);
  if (threadIdx.x == 0) S.kin0[blockIdx.x] = k;
}

enum HmcLeap : int { kLeapFirst = 0, kLeapMiddle = 1, kLeapLast = 2 };

// first:  p ← p − ½s·g_cur, q ← q + s·p       (g_cur = ∇U(θ), the cache)
// middle: g = hmc_grad at q; p ← p − s·g, q ← q + s·p
// last:   g = hmc_grad at q; p ← p − ½s·g; g_new ← g; kin1, prior[workgroup] = Σ p², Σ q²
template <int KIND>
__global__ __launch_bounds__(kNT) void hmc_leap_kernel(const HmcDev S, const double* __restrict__ part_theta,
                                                       int nblk, double s) {
  __shared__ double red[kNW];
  if (hmc_stopped(S.status)) return;
  const size_t nC = (size_t)S.n * S.C;
  const size_t e = (size_t)blockIdx.x * kNT + threadIdx.x;
  double p = 0.0, q = 0.0;
  if (e < nC) {
    q = S.q[e];
    const double g = KIND == kLeapFirst ? S.g_cur[e] : hmc_grad(part_theta, nblk, nC, e, q);
    const double sp = KIND == kLeapMiddle ? s : __dmul_rn(0.5, s);
    p = __dsub_rn(S.p[e], __dmul_rn(sp, g));
    S.p[e] = p;
    if constexpr (KIND != kLeapLast) {
      q = __dadd_rn(q, __dmul_rn(s, p));
      S.q[e] = q;
    } else {
      S.g_new[e] = g;
    }
  }
  if constexpr (KIND == kLeapLast) {
    const double k = blk_sum(__dmul_rn(p, p), red), t2 = blk_sum(__dmul_rn(q, q), red);
    if (threadIdx.x == 0) {
      S.kin1[blockIdx.x] = k;
      S.prior[blockIdx.x] = t2;
    }
  }
}

// The cache of a run's first state, after an evaluation at θ: g_cur = ∇U(θ) and the ‖θ‖² partials.
__global__ __launch_bounds__(kNT) void hmc_prime_kernel(const HmcDev S, const double* __restrict__ part_theta,
                                                        int nblk) {
  __shared__ double red[kNW];
  if (hmc_stopped(S.status)) return;
  const size_t nC = (size_t)S.n * S.C;
  const size_t e = (size_t)blockIdx.x * kNT + threadIdx.x;
  double q = 0.0;
  if (e < nC) {
    q = S.theta[e];
    S.g_cur[e] = hmc_grad(part_theta, nblk, nC, e, q);
  }
  const double t2 = blk_sum(__dmul_rn(q, q), red);
  if (threadIdx.x == 0) S.prior[blockIdx.x] = t2;
}

// U = Σ_b value partials + ½ Σ_b ‖·‖² partials, both in workgroup order (sh: the partials in LDS).
static __device__ __forceinline__ double hmc_potential(const double* val, int nblk, const double* pri,
                                                       int nb) {
  double v = 0.0, t2 = 0.0;
  for (int b = 0; b < nblk; ++b) v += val[b];
  for (int b = 0; b < nb; ++b) t2 += pri[b];
  return __dadd_rn(v, __dmul_rn(0.5, t2));
}
static __device__ __forceinline__ double hmc_kinetic(const double* kin, int nb) {
  double k = 0.0;
  for (int b = 0; b < nb; ++b) k += kin[b];
  return __dmul_rn(0.5, k);
}

enum HmcDecide : int { kDecPrime = 0, kDecDecide = 1, kDecReport = 2 };

// One workgroup; the partials come into LDS by all threads and thread 0 adds them in order.
//   prime:  sc[0] = U(θ) from the evaluation at θ and hmc_prime_kernel's partials;
//   decide: H0 = sc[0] + ½Σkin0, H1 = U(q) + ½Σkin1, u = the uniform of (seed, t, kHmcAccept, 0);
//           accept iff H1 is finite and u < exp(H0 − H1) (an overflowing exponent is +inf and
//           accepts); flag ← accept, sc[0] ← U(q) on accept; record i of the call: accept, H0 − H1,
//           U of the kept state; a non-finite H1 adds one to *ndiv;
//   report: sc[2] = H0, sc[3] = H1, nothing else (the integrator alone).
template <int MODE>
__global__ __launch_bounds__(kNT) void hmc_decide_kernel(const HmcDev S, const double* __restrict__ part_sc,
                                                         int nblk, int nb, uint64_t seed, uint32_t t,
                                                         long long i, int32_t* __restrict__ acc_rec,
                                                         double* __restrict__ dh_rec,
                                                         double* __restrict__ val_rec) {
  __shared__ double val[kCjMaxBlocks], pri[kHmcMaxBlocks], k0[kHmcMaxBlocks], k1[kHmcMaxBlocks];
  if (hmc_stopped(S.status)) return;
  for (int b = threadIdx.x; b < nblk; b += kNT) val[b] = part_sc[2 * b];
  for (int b = threadIdx.x; b < nb; b += kNT) {
    pri[b] = S.prior[b];
    if constexpr (MODE != kDecPrime) {
      k0[b] = S.kin0[b];
      k1[b] = S.kin1[b];
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double U = hmc_potential(val, nblk, pri, nb);
  if constexpr (MODE == kDecPrime) {
    S.sc[0] = U;
  } else {
    const double H0 = __dadd_rn(S.sc[0], hmc_kinetic(k0, nb));
    const double H1 = __dadd_rn(U, hmc_kinetic(k1, nb));
    if constexpr (MODE == kDecReport) {
      S.sc[2] = H0;
      S.sc[3] = H1;
    } else {
      const double dH = __dsub_rn(H0, H1);
      const bool finite = fabs(H1) <= DBL_MAX;
      const U4 x = philox4x32(0u, t, kHmcAccept, 0u, seed);
      const bool acc = finite && u53(x.x, x.y) < exp(dH);
      S.flag[0] = acc ? 1 : 0;
      if (acc) S.sc[0] = U;
      if (!finite) S.ndiv[0] += 1;
      acc_rec[i] = acc ? 1 : 0;
      dh_rec[i] = dH;
      val_rec[i] = acc ? U : S.sc[0];
    }
  }
}

// θ ← q and g_cur ← g_new where the decision accepted; store_col (n·C, or null) takes the kept θ.
__global__ __launch_bounds__(kNT) void hmc_commit_kernel(const HmcDev S, double* __restrict__ store_col) {
  if (hmc_stopped(S.status)) return;
  const size_t nC = (size_t)S.n * S.C;
  const size_t e = (size_t)blockIdx.x * kNT + threadIdx.x;
  if (e >= nC) return;
  const bool acc = S.flag[0] != 0;
  if (acc) {
    const double q = S.q[e];
    S.theta[e] = q;
    S.g_cur[e] = S.g_new[e];
    if (store_col) store_col[e] = q;
  } else if (store_col) {
    store_col[e] = S.theta[e];
  }
}

int hmc_blocks(int n, int C) { return (int)(((size_t)n * C + kNT - 1) / kNT); }

static bool hmc_shape_ok(const HmcDev& S, int nblk) {
  const int nb = hmc_blocks(S.n, S.C);
  return S.n >= 1 && S.C >= 1 && nb >= 1 && nb <= kHmcMaxBlocks && nblk >= 1 && nblk <= kCjMaxBlocks;
}

hipError_t launch_hmc_begin(const HmcDev& S, bool draw, uint64_t seed, uint32_t t, hipStream_t st) {
  if (!hmc_shape_ok(S, 1)) return hipErrorInvalidValue;
  const dim3 grid(hmc_blocks(S.n, S.C));
  if (draw) hipLaunchKernelGGL(hmc_begin_kernel<true>, grid, dim3(kNT), 0, st, S, seed, t);
  else hipLaunchKernelGGL(hmc_begin_kernel<false>, grid, dim3(kNT), 0, st, S, seed, t);
  return hipGetLastError();
}

hipError_t launch_hmc_leap(const HmcDev& S, int kind, const double* part_theta, int nblk, double s,
                           hipStream_t st) {
  if (!hmc_shape_ok(S, nblk)) return hipErrorInvalidValue;
  const dim3 grid(hmc_blocks(S.n, S.C));
  return with_value(IntList<kLeapFirst, kLeapMiddle, kLeapLast>{}, kind, [&](auto KIND) {
    hipLaunchKernelGGL(hmc_leap_kernel<KIND>, grid, dim3(kNT), 0, st, S, part_theta, nblk, s);
    return hipGetLastError();
  });
}

hipError_t launch_hmc_prime(const HmcDev& S, const double* part_theta, int nblk, hipStream_t st) {
  if (!hmc_shape_ok(S, nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hmc_prime_kernel, dim3(hmc_blocks(S.n, S.C)), dim3(kNT), 0, st, S, part_theta,
                     nblk);
  return hipGetLastError();
}

hipError_t launch_hmc_decide(const HmcDev& S, int mode, const double* part_sc, int nblk,
                             uint64_t seed, uint32_t t, long long i, int32_t* acc_rec,
                             double* dh_rec, double* val_rec, hipStream_t st) {
  if (!hmc_shape_ok(S, nblk)) return hipErrorInvalidValue;
  const int nb = hmc_blocks(S.n, S.C);
  return with_value(IntList<kDecPrime, kDecDecide, kDecReport>{}, mode, [&](auto MODE) {
    hipLaunchKernelGGL(hmc_decide_kernel<MODE>, dim3(1), dim3(kNT), 0, st, S, part_sc, nblk, nb,
                       seed, t, i, acc_rec, dh_rec, val_rec);
    return hipGetLastError();
  });
}

hipError_t launch_hmc_commit(const HmcDev& S, double* store_col, hipStream_t st) {
  if (!hmc_shape_ok(S, 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hmc_commit_kernel, dim3(hmc_blocks(S.n, S.C)), dim3(kNT), 0, st, S, store_col);
  return hipGetLastError();
}

}  // namespace gpt
