// Random-Fourier-feature maps (GPT_SGLD.jl:71-84, 109-120) and the full-theta SGLD step
// (GPNT_SGLD, GPT_SGLD.jl:809-847).
#include "device_util.h"

namespace gpt {

// phi[j + n(k + D i)] = c · cos(X[i + N k] · (Z[j + n k] · (1/ls[k])) + b[j + n k]).
// The argument is formed with round-to-nearest multiplies/adds (no FMA contraction) so it is
// the same double the reference forms; only cos differs (≤1 ulp between libms).
__global__ __launch_bounds__(256) void feature_kernel(const double* __restrict__ X, long long N,
                                                      int D, const double* __restrict__ ls,
                                                      double c, const double* __restrict__ Z,
                                                      const double* __restrict__ b, int n,
                                                      double* __restrict__ phi) {
  const long long total = (long long)n * D * N;
  for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < total;
       x += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(x % n);
    const long long rest = x / n;
    const int k = (int)(rest % D);
    const long long i = rest / D;
    const double zt = __dmul_rn(Z[j + (long long)n * k], 1.0 / ls[k]);
    const double arg = __dadd_rn(__dmul_rn(X[i + N * k], zt), b[j + (long long)n * k]);
    phi[x] = c * cos(arg);
  }
}

// phi[j + n i] = c · cos(Σ_k X[i,k]·Zt[j,k] + b[j]),  c = sqrt(2/n)·σ  (sum in k order).
__global__ __launch_bounds__(256) void feature_notensor_kernel(
    const double* __restrict__ X, long long N, int D, const double* __restrict__ ls, double c,
    const double* __restrict__ Z, const double* __restrict__ b, int n, double* __restrict__ phi) {
  const long long total = (long long)n * N;
  for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < total;
       x += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(x % n);
    const long long i = x / n;
    double s = 0.0;
    for (int k = 0; k < D; ++k)
      s = __dadd_rn(s, __dmul_rn(X[i + N * k], __dmul_rn(Z[j + (long long)n * k], 1.0 / ls[k])));
    phi[x] = c * cos(__dadd_rn(s, b[j]));
  }
}

hipError_t launch_feature(const double* X, long long N, int D, const double* ls, double c,
                          const double* Z, const double* b, int n, double* phi, hipStream_t st) {
  const long long total = (long long)n * D * N;
  const int blocks = (int)min((total + 255) / 256, (long long)256 * 16);
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(feature_kernel, dim3(blocks), dim3(256), 0, st, X, N, D, ls, c, Z, b, n, phi);
  return hipGetLastError();
}

hipError_t launch_feature_notensor(const double* X, long long N, int D, const double* ls,
                                   double c, const double* Z, const double* b, int n,
                                   double* phi, hipStream_t st) {
  const long long total = (long long)n * N;
  const int blocks = (int)min((total + 255) / 256, (long long)256 * 16);
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(feature_notensor_kernel, dim3(blocks), dim3(256), 0, st, X, N, D, ls, c, Z,
                     b, n, phi);
  return hipGetLastError();
}

// The stager of X-mode sessions (gpt_sgld_session_create_x): the feature rows, targets and view
// entries of whole minibatches into a chain's ring (gpt_internal.h StageParams), so that no
// n·D·N phi exists (kin40kExperiment.jl:67-74: every sweep's phi differs only in length_scale and
// sigma_RBF).  One workgroup per (chain, dimension k, batch, group of kStageRows rows): lanes over
// j keep zt = Z[j,k]·(1/ls_c[k]) and b[j,k] in registers across the rows, X[row,k] is one
// wave-uniform scalar per row, and every row's n doubles go out as one coalesced run.  Each
// feature is feature_kernel's double: c·cos(x·zt + b) with round-to-nearest multiply and add and
// the library cos, so an X-mode trajectory is the phi-mode trajectory bit for bit.  The step
// counter comes from the device (captured graphs replay), and a batch at or past total_steps is
// skipped: no step reads it and its epoch's order may not exist.
constexpr int kStageRows = 8;
__global__ __launch_bounds__(256) void stage_batches_kernel(const StageParams S,
                                                            const ChainDesc* __restrict__ real,
                                                            const ChainDesc* __restrict__ view,
                                                            const long long* __restrict__ tbase,
                                                            int t_first) {
  const int c = blockIdx.z, k = blockIdx.y;
  const int ngrp = (S.m + kStageRows - 1) / kStageRows;
  const int q = blockIdx.x / ngrp, g = blockIdx.x - q * ngrp;
  const long long t = tbase[0] + t_first + q;
  if (t >= S.total_steps) return;
  const int e = (int)(t / S.nb), bb = (int)(t - (long long)e * S.nb);
  const int Bt = min(S.m, S.N - bb * S.m);
  const int i0 = g * kStageRows, i1 = min(Bt, i0 + kStageRows);
  if (i0 >= Bt) return;
  const int slot = (int)(t % S.KR);
  const int n = S.n, N = S.N;
  const size_t at = (size_t)(e & 1) * N + (size_t)bb * S.m;        // the batch in an order ring
  const int32_t* ord = real[c].order + at;
  double* ring = (double*)view[c].phi + (size_t)slot * S.m * n * S.D + (size_t)n * k;
  const double* Xk = S.X + (size_t)N * k;
  const double inv = 1.0 / S.ls[(size_t)S.ls_len * c + (S.ls_len == 1 ? 0 : k)];
  const double cc = S.cfeat[c];
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const double zt = __dmul_rn(S.Z[j + (size_t)n * k], inv);
    const double bj = S.b[j + (size_t)n * k];
#pragma unroll 1
    for (int i = i0; i < i1; ++i) {
      const int row = min(max(ord[i], 0), N - 1);                   // in range whatever the ring holds
      ring[(size_t)i * n * S.D + j] = cc * cos(__dadd_rn(__dmul_rn(Xk[row], zt), bj));
    }
  }
  if (k == 0) {
    double* yr = (double*)view[c].y + (size_t)slot * S.m;
    int32_t* rows = (int32_t*)((char*)view[c].phi + S.o_rows) + (size_t)slot * S.m;
    int32_t* vw = view[c].order + at;
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
      const int row = min(max(ord[i], 0), N - 1);
      yr[i] = real[c].y[row];
      rows[i] = row;
      vw[i] = slot * S.m + i;
    }
  }
}

hipError_t launch_stage_batches(const StageParams& S, const ChainDesc* real, const ChainDesc* view,
                                int nchains, const long long* tbase, int t_first, int count,
                                hipStream_t st) {
  if (count < 1 || nchains < 1) return hipSuccess;
  if (nchains > 65535 || S.D > 65535 || count > S.KR) return hipErrorInvalidValue;
  const int ngrp = (S.m + kStageRows - 1) / kStageRows;
  const int nt = min(256, (S.n + 63) / 64 * 64);
  hipLaunchKernelGGL(stage_batches_kernel, dim3((unsigned)(count * ngrp), S.D, nchains), dim3(nt),
                     0, st, S, real, view, tbase, t_first);
  return hipGetLastError();
}

// One full-theta SGLD step (GPT_SGLD.jl:826-843) in one workgroup:
//   res = y_B − Φ_Bᵀθ ;  θ += ε_t/2·(−θ/σθ² + (N/B)Φ_B res/σ²) + sqrt(ε_t)·ξ ;  store θ.
__global__ __launch_bounds__(kNT) void gpnt_step_kernel(
    const double* __restrict__ phi, const double* __restrict__ y,
    const int32_t* __restrict__ order, int n, int N, int m, int nb, long long total,
    double signal_var, double sigma_theta, double eps_theta, double decay_rate, uint64_t seed,
    double* __restrict__ theta, double* __restrict__ store, int32_t* __restrict__ status,
    const long long* __restrict__ tbase, int t_local) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const long long t = tbase[0] + t_local;
  if (t >= total) return;
  if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int e = (int)(t / nb), b = (int)(t - (long long)e * nb);
  const int start = b * m;
  const int Bt = min(m, N - start);
  int* idx_l = (int*)smem;
  double* res_l = (double*)(smem + al16(4 * (size_t)m));
  double* red = res_l + ((m + 1) & ~1);
  const int32_t* ord = order + (size_t)e * N + start;
  for (int i = tid; i < Bt; i += kNT) idx_l[i] = ord[i];
  __syncthreads();
  // Φ_Bᵀθ: lanes over features j (coalesced), 64 batch columns per pass, Butterfly over lanes.
  for (int base = 0; base < Bt; base += 64) {
    double v[64];
#pragma unroll
    for (int u = 0; u < 64; ++u) v[u] = 0.0;
    for (int j = wv * 64 + lane; j < n; j += kNT) {
      const double th = theta[j];
#pragma unroll
      for (int u = 0; u < 64; ++u) {
        const int i = min(base + u, Bt - 1);
        v[u] = fma(phi[(long long)uni(idx_l[i]) * n + j], th, v[u]);
      }
    }
    Butterfly<64>::run(v, lane);
    red[wv * 64 + lane] = v[0];
    __syncthreads();
    if (tid < 64 && base + tid < Bt) {
      double s = 0.0;
#pragma unroll
      for (int w2 = 0; w2 < kNW; ++w2) s += red[w2 * 64 + tid];
      res_l[base + tid] = y[idx_l[base + tid]] - s;
    }
    __syncthreads();
  }
  const double eps = eps_theta * pow((double)(t + 1), -decay_rate);
  const double cN = (double)N / (double)Bt;
  const double isg2 = 1.0 / (sigma_theta * sigma_theta);
  bool bad = false;
  double* out = store ? store + (size_t)t * n : nullptr;
  for (int j = tid; j < n; j += kNT) {
    double g = 0.0;
    for (int i = 0; i < Bt; ++i) g = fma(phi[(long long)uni(idx_l[i]) * n + j], res_l[i], g);
    const double th = theta[j];
    const double grad = -th * isg2 + cN * g / signal_var;
    const double nt = th + (eps * grad / 2 +
                            sqrt(eps) * normal_at(seed, (uint32_t)j, (uint32_t)t, kThetaNoise, 0));
    theta[j] = nt;
    if (out) out[j] = nt;
    bad |= (nt != nt);
  }
  if (__syncthreads_or(bad) && tid == 0)
    __hip_atomic_store(status, GPT_ERR_NAN_THETA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_gpnt(const double* phi, const double* y, const int32_t* order, int n, int N,
                       int m, int nb, long long total, double signal_var, double sigma_theta,
                       double eps_theta, double decay_rate, uint64_t seed, double* theta,
                       double* theta_store, int32_t* status, const long long* tbase, int t_local,
                       hipStream_t st) {
  const size_t lds = al16(4 * (size_t)m) + 8 * (size_t)(((m + 1) & ~1) + kNW * 64);
  hipLaunchKernelGGL(gpnt_step_kernel, dim3(1), dim3(kNT), lds, st, phi, y, order, n, N, m, nb,
                     total, signal_var, sigma_theta, eps_theta, decay_rate, seed, theta,
                     theta_store, status, tbase, t_local);
  return hipGetLastError();
}

}  // namespace gpt
