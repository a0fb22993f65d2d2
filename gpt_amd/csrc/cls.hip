// Classification on the device: the full-theta softmax sampler (GPNT_SGLDclass,
// GPT_SGLD.jl:851-901), the scores of stored full-theta samples (ImageNoTensorExperiment.jl:55)
// and the evaluation of class scores: miss rate and mean negative log predictive probability
// per sample and on the scores averaged over a window of samples (ImageExperiment.jl:50-72,
// ImageNoTensorExperiment.jl:50-75).  Everything is fp64; exp and log are the device library's.
#include "gpt_internal.h"
#include "theta_chain.h"

namespace gpt {

// ------------------------------------------------------------------ GPNT_SGLDclass
// LDS of ntc_chain_kernel: theta (CC columns of n, the columns past C stay zero), the batch's row
// numbers and 0-based labels, the C x B residual, and the batch's n x B features when they fit.
NtcLayout ntc_layout(int n, int C, int m) {
  NtcLayout L;
  L.CC = C <= 2 ? 2 : (C <= 4 ? 4 : (C <= 8 ? 8 : (C <= 16 ? 16 : 32)));
  size_t o = 0;
  L.o_theta = o; o = al16(o + 8 * (size_t)n * L.CC);
  L.o_idx = o;   o = al16(o + 4 * (size_t)m);
  L.o_yb = o;    o = al16(o + 4 * (size_t)m);
  L.o_P = o;     o = al16(o + 8 * (size_t)C * m);
  L.o_flag = o;  o = al16(o + 4 * (size_t)kNW);
  L.o_phi = o;
  L.base = o;
  const size_t staged = al16(o + 8 * (size_t)n * m);
  L.stage = staged <= (size_t)kMaxLds ? 1 : 0;
  L.bytes = L.stage ? staged : o;
  return L;
}

// One workgroup per chain runs steps t0 .. t0+nsteps-1 (0-based, within one epoch) with theta in
// LDS; theta goes to HBM on store steps and at the end of the launch.  Per step (:869-899):
//   x = thetaᵀ·Φ_B (one wave per batch column, lanes over j, CC accumulators, one wave_sum each),
//   P = softmax(x) per column with P[y_i, i] −= 1,
//   grad = (N/B)·Φ_B·Pᵀ + θ (lanes over j, P read by broadcast, i in order),
//   θ −= ε_t/2·grad + sqrt(ε_t)·ξ.
// Every sum has a fixed order, and every exit is taken by the whole workgroup.
template <int CC>
__global__ __launch_bounds__(kNT) void ntc_chain_kernel(
    const double* __restrict__ phi, const int32_t* __restrict__ y0,
    const NtcChain* __restrict__ chains, int n, int N, int C, int m, int nb, long long total,
    double decay_rate, int store_every, long long t0, int nsteps, NtcLayout L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const NtcChain ch = chains[blockIdx.x];
  if (theta_chain_done(t0, total, ch.status)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
  double* theta_l = (double*)(smem + L.o_theta);
  int* idx_l = (int*)(smem + L.o_idx);
  int* yb_l = (int*)(smem + L.o_yb);
  double* P_l = (double*)(smem + L.o_P);
  double* phi_l = (double*)(smem + L.o_phi);
  int* flag_l = (int*)(smem + L.o_flag);
  const int stage = L.stage;
  for (int e = tid; e < n * CC; e += kNT) theta_l[e] = e < n * C ? ch.theta[e] : 0.0;
  const int NP = ((n + 63) / 64) * 64;
  const long long tend = min(total, t0 + (long long)nsteps);
  for (long long t = t0; t < tend; ++t) {
    const int32_t* ord;
    const int Bt = theta_batch(ch.order, t, nb, m, N, &ord);
    __syncthreads();                          // theta_l loaded / the step before is finished
    gather_batch(ord, Bt, N, y0, idx_l, yb_l);
    __syncthreads();
    for (int i = wv; i < Bt; i += kNW) {
      const double* col = phi + (long long)uni(idx_l[i]) * n;
      double acc[CC];
#pragma unroll
      for (int c = 0; c < CC; ++c) acc[c] = 0.0;
      for (int j = lane; j < n; j += 64) {
        const double pv = col[j];
        if (stage) phi_l[(size_t)i * n + j] = pv;
#pragma unroll
        for (int c = 0; c < CC; ++c) acc[c] = fma(pv, theta_l[c * n + j], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < CC; ++c) acc[c] = wave_sum(acc[c]);
      double a = acc[0];
#pragma unroll
      for (int c = 1; c < CC; ++c)
        if (c < C) a = fmax(a, acc[c]);
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) s += exp(acc[c] - a);
      const double lse = a + log(s);
      const int yi = uni(yb_l[i]);
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C && lane == c) P_l[c * m + i] = exp(acc[c] - lse) - (c == yi ? 1.0 : 0.0);
    }
    __syncthreads();
    const ThetaStepSize S = theta_step_size(ch.eps_theta, t, decay_rate, N, Bt);
    const double eps = S.eps, sq = S.sq, cN = S.cN;
    double* out = theta_store_slot(ch.store, t, store_every, (size_t)n * C);
    bool bad = false;
    for (int e = tid; e < NP * C; e += kNT) {
      const int c = e / NP, j = e - c * NP;   // c is uniform over a wave: P_l is read by broadcast
      if (j >= n) continue;
      const double* Pc = P_l + c * m;
      double g = 0.0;
      if (stage) {
        for (int i = 0; i < Bt; ++i) g = fma(phi_l[(size_t)i * n + j], Pc[i], g);
      } else {
        for (int i = 0; i < Bt; ++i) g = fma(phi[(long long)idx_l[i] * n + j], Pc[i], g);
      }
      const double th = theta_l[c * n + j];
      const double grad = cN * g + th;
      const double xi = normal_at(ch.seed, (uint32_t)j, (uint32_t)t, kThetaNoise, (uint32_t)c);
      const double nt = th - (eps * grad / 2 + sq * xi);
      theta_l[c * n + j] = nt;
      if (out) out[c * n + j] = nt;
      bad |= (nt != nt);
    }
    if (theta_chain_nan(bad, flag_l, ch.status)) return;
  }
  __syncthreads();
  for (int e = tid; e < n * C; e += kNT) ch.theta[e] = theta_l[e];
}

hipError_t launch_ntc_chain(const double* phi, const int32_t* y0, const NtcChain* chains,
                            int nchains, int n, int N, int C, int m, int nb, long long total,
                            double decay_rate, int store_every, long long t0, int nsteps,
                            const NtcLayout& L, hipStream_t st) {
  if (C < 1 || C > 32 || L.bytes > (size_t)kMaxLds || nchains < 1 || store_every < 1)
    return hipErrorInvalidValue;
  const int cc = contains(IntList<2, 4, 8, 16>{}, L.CC) ? L.CC : 32;    // C rounded up
  return with_value(IntList<2, 4, 8, 16, 32>{}, cc, [&](auto CC) {
    return launch_lds_over_64k<ntc_chain_kernel<CC>>(
        kMaxLds, dim3(nchains), dim3(kNT), L.bytes, st, phi, y0, chains, n, N, C, m, nb, total,
        decay_rate, store_every, t0, nsteps, L);
  });
}

// ------------------------------------------------------------------ scores of full-theta samples
// scores[i + Ntest·s] = Σ_j phitest[j, i]·theta[j, s], s = c + C·t over the stacked samples.
// Register-tiled: a 64 x 64 tile per workgroup of 256 threads (4 x 4 per thread), K in chunks of
// 16 through LDS.  Every output is one fma chain over j in order, whatever the tiling.
constexpr int kScT = 64, kScK = 16;
__global__ __launch_bounds__(256) void nt_scores_kernel(
    const double* __restrict__ phitest, const double* __restrict__ theta, int n, long long Ntest,
    long long S, double* __restrict__ scores) {
  __shared__ double As[kScK][kScT + 1], Bs[kScK][kScT + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long i0 = (long long)blockIdx.x * kScT, s0 = (long long)blockIdx.y * kScT;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int k0 = 0; k0 < n; k0 += kScK) {
    for (int e = tid; e < kScK * kScT; e += 256) {
      const int k = e & (kScK - 1), x = e >> 4;
      const bool kin = k0 + k < n;
      As[k][x] = (kin && i0 + x < Ntest) ? phitest[(size_t)(i0 + x) * n + k0 + k] : 0.0;
      Bs[k][x] = (kin && s0 + x < S) ? theta[(size_t)(s0 + x) * n + k0 + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kScK; ++k) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = As[k][tx + 16 * a];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = Bs[k][ty + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const long long s = s0 + ty + 16 * b;
    if (s >= S) continue;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const long long i = i0 + tx + 16 * a;
      if (i < Ntest) scores[(size_t)s * Ntest + i] = acc[a][b];
    }
  }
}

hipError_t launch_nt_scores(const double* phitest, const double* theta, int n, long long Ntest,
                            long long S, double* scores, hipStream_t st) {
  if (Ntest < 1 || S < 1) return hipSuccess;
  const long long gx = (Ntest + kScT - 1) / kScT, gy = (S + kScT - 1) / kScT;
  if (gx > 0x7fffffffLL || gy > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nt_scores_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, phitest,
                     theta, n, Ntest, S, scores);
  return hipGetLastError();
}

// ------------------------------------------------------------------ evaluation of scores
// One thread per row of a tile of kEvalRows rows, one sample per blockIdx.y (strided):
//   a = max_c x, lse = a + log Σ_c exp(x − a), nlp = lse − x[y], prediction = first index of a.
// A tile's nlp sum is one wave_sum per wave and the waves in order; misses are integers.  The tile
// size is fixed, so the partial sums (and class_finish_kernel's sum over them in tile order) do
// not depend on the launch.
constexpr int kEvalRows = 256;
__global__ __launch_bounds__(kEvalRows) void class_eval_kernel(
    const double* __restrict__ scores, const int32_t* __restrict__ y, long long Ntest, int C, int T,
    double* __restrict__ part_nlp, int32_t* __restrict__ part_miss, int32_t* __restrict__ pred_out,
    double* __restrict__ nlp_out) {
  __shared__ double red[kEvalRows / 64];
  __shared__ int redm[kEvalRows / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long i = (long long)blockIdx.x * kEvalRows + tid;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    double nlp = 0.0;
    int miss = 0;
    if (i < Ntest) {
      const double* x = scores + (size_t)t * C * Ntest + i;
      double a = x[0];
      int arg = 0;
      for (int c = 1; c < C; ++c) {
        const double v = x[(size_t)c * Ntest];
        if (v > a) { a = v; arg = c; }
      }
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += exp(x[(size_t)c * Ntest] - a);
      const int yi = min(max(y[i] - 1, 0), C - 1);       // labels are checked on the host
      nlp = (a + log(s)) - x[(size_t)yi * Ntest];
      miss = arg != yi;
      if (pred_out) pred_out[(size_t)t * Ntest + i] = arg + 1;
      if (nlp_out) nlp_out[(size_t)t * Ntest + i] = nlp;
    }
    const double ws = wave_sum(nlp);
    const int wm = __popcll(__ballot(miss));
    if (lane == 0) { red[wv] = ws; redm[wv] = wm; }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      int mm = 0;
      for (int w = 0; w < kEvalRows / 64; ++w) { s += red[w]; mm += redm[w]; }
      part_nlp[(size_t)t * gridDim.x + blockIdx.x] = s;
      part_miss[(size_t)t * gridDim.x + blockIdx.x] = mm;
    }
    __syncthreads();
  }
}

// prop_missed[t] = 1 − hits/Ntest, mean_nlp[t] = (Σ tiles in order)/Ntest
__global__ void class_finish_kernel(const double* __restrict__ part_nlp,
                                    const int32_t* __restrict__ part_miss, int ntiles, int T,
                                    long long Ntest, double* __restrict__ prop_missed,
                                    double* __restrict__ mean_nlp) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  double s = 0.0;
  long long mm = 0;
  for (int k = 0; k < ntiles; ++k) {
    s += part_nlp[(size_t)t * ntiles + k];
    mm += part_miss[(size_t)t * ntiles + k];
  }
  prop_missed[t] = 1.0 - (double)(Ntest - mm) / (double)Ntest;
  mean_nlp[t] = s / (double)Ntest;
}

// mean over the samples first .. last-1 of every (row, class), summed in sample order
__global__ __launch_bounds__(256) void class_mean_kernel(const double* __restrict__ scores,
                                                         long long rows, int first, int last,
                                                         double* __restrict__ mean_out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows) return;
  double s = 0.0;
  for (int t = first; t < last; ++t) s += scores[(size_t)t * rows + e];
  mean_out[e] = s / (double)(last - first);
}

size_t class_eval_tiles(long long Ntest) { return (size_t)((Ntest + kEvalRows - 1) / kEvalRows); }

hipError_t launch_class_eval(const double* scores, const int32_t* y, long long Ntest, int C, int T,
                             double* part_nlp, int32_t* part_miss, double* prop_missed,
                             double* mean_nlp, int32_t* pred_out, double* nlp_out, hipStream_t st) {
  const size_t ntiles = class_eval_tiles(Ntest);
  if (ntiles < 1 || ntiles > 0x7fffffffULL || T < 1 || C < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(class_eval_kernel, dim3((unsigned)ntiles, (unsigned)min(T, 65535)),
                     dim3(kEvalRows), 0, st, scores, y, Ntest, C, T, part_nlp, part_miss, pred_out,
                     nlp_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(class_finish_kernel, dim3((T + 63) / 64), dim3(64), 0, st, part_nlp, part_miss,
                     (int)ntiles, T, Ntest, prop_missed, mean_nlp);
  return hipGetLastError();
}

hipError_t launch_class_mean(const double* scores, long long Ntest, int C, int first, int last,
                             double* mean_out, hipStream_t st) {
  const long long rows = Ntest * C;
  const long long g = (rows + 255) / 256;
  if (g < 1 || g > 0x7fffffffLL || first < 0 || last <= first) return hipErrorInvalidValue;
  hipLaunchKernelGGL(class_mean_kernel, dim3((unsigned)g), dim3(256), 0, st, scores, rows, first,
                     last, mean_out);
  return hipGetLastError();
}

}  // namespace gpt
