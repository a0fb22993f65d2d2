// The frame of the full-theta chain kernels (gpnt_chain_kernel, ntc_chain_kernel): one workgroup
// per ThetaChain runs steps t0 .. t0+nsteps-1 with theta in LDS.  What a step does to theta is
// the kernel's own; the rest of a step is here, once.
#pragma once
#include "device_util.h"

namespace gpt {

// Nothing to do for this launch: the steps are past the run's end, or the chain met a NaN before.
__device__ __forceinline__ bool theta_chain_done(long long t0, long long total,
                                                 const int32_t* status) {
  return t0 >= total ||
         __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// Batch b = t mod nb of epoch ep = t / nb: the Bt rows numbered by (*ord)[0 .. Bt) (GPT_SGLD.jl:826-829).
__device__ __forceinline__ int theta_batch(const int32_t* order, long long t, int nb, int m, int N,
                                           const int32_t** ord) {
  const int ep = (int)(t / nb), b = (int)(t - (long long)ep * nb);
  const int start = b * m;
  *ord = order + (size_t)ep * N + start;
  return min(m, N - start);
}
// Its row numbers, clamped to the data, into idx_l and each row's target or label into yb_l.
template <class Y>
__device__ __forceinline__ void gather_batch(const int32_t* ord, int Bt, int N,
                                             const Y* __restrict__ y, int* idx_l, Y* yb_l) {
  for (int i = threadIdx.x; i < Bt; i += kNT) {
    const int row = min(max(ord[i], 0), N - 1);
    idx_l[i] = row;
    yb_l[i] = y[row];
  }
}

// Step t (0-based): eps = eps_theta·(t+1)^-decay_rate, sq = sqrt(eps), cN = N / Bt.
struct ThetaStepSize {
  double eps, sq, cN;
};
__device__ __forceinline__ ThetaStepSize theta_step_size(double eps_theta, long long t,
                                                         double decay_rate, int N, int Bt) {
  const double eps = eps_theta * pow((double)(t + 1), -decay_rate);
  return {eps, sqrt(eps), (double)N / (double)Bt};
}
// Where its theta (len doubles) goes: the 1-based steps divisible by store_every are kept.
__device__ __forceinline__ double* theta_store_slot(double* store, long long t, int store_every,
                                                    size_t len) {
  const bool keep = ((t + 1) % store_every) == 0;
  return keep ? store + (size_t)((t + 1) / store_every - 1) * len : nullptr;
}

// True, with the chain's status set, when a lane of the workgroup saw a NaN in its new theta.
// The whole workgroup leaves together: a flag per wave in dynamic LDS (no static LDS, so the
// kernel's dynamic limit can be the full 160 KB)
__device__ __forceinline__ bool theta_chain_nan(bool bad, int* flag_l, int32_t* status) {
  const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
  const int wbad = __ballot(bad) != 0 ? 1 : 0;
  if (lane == 0) flag_l[wv] = wbad;
  __syncthreads();
  int any = 0;
#pragma unroll
  for (int w2 = 0; w2 < kNW; ++w2) any |= flag_l[w2];
  if (__builtin_expect(any == 0, 1)) return false;      // the step's usual end
  if (tid == 0)
    __hip_atomic_store(status, GPT_ERR_NAN_THETA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

}  // namespace gpt
