// Chain diagnostics of a store x[p, s, m] (parameter or test row p, kept sample s, chain m): split
// R-hat, the combined autocorrelation, Geyer's initial-monotone-sequence tau, ESS and MCSE over the
// window's S samples.  Column-major (P, T, M): element (p, s, m) at x + p + P·s + cstride·m, so the
// 64 lanes of a wave are 64 neighbouring parameters and a sample row is one 512-byte read.
//
// Three kernels, every sum in an order that S and K alone fix:
//   diag_mean_kernel     one lane per (p, m), the S samples in order: chain_mean = (Σ x)/S, and in
//                        deviations from the chain's first sample x0 (exact where the samples agree,
//                        and a common offset gone before anything is squared) ebar = (Σ (x − x0))/S
//                        and the same mean over the first and the last H = ⌊S/2⌋ samples.
//   diag_acov_kernel     one workgroup per (64 parameters, group of kKG lags), the chains in order
//                        m = 0 … M − 1 inside it.  Per chain it walks the window in chunks of kTC
//                        samples: the centred values c = (x − x0) − ebar of the chunk and of its
//                        halo go to LDS once, and wave w keeps the kKB lags 1 + kKG·g + kKB·w … in
//                        registers, kSB samples × kKB lags per block: kSB + (kSB + kKB − 1) LDS reads
//                        for kSB·kKB fused multiply-adds.  Lag k's sum is one chain s = 0 … S − 1 − k
//                        whatever the tiling (samples past the window enter as c = 0: fma(c, 0, a) is
//                        a).  Wave 0 of group 0 also keeps lag 0 and the two half-chain sums of
//                        squares about the half means.  acov_m(k) = sum/S; Σ_m acov_m(k) in chain
//                        order, /M, is the only thing stored per lag: P·(K + 1) doubles.
//   diag_finish_kernel   one lane per parameter: W, B/S, var+, acf, the Geyer walk and split R-hat.
// No atomics and no scratch; a parameter's results depend on its own values alone, a chain's
// mean, variance and acov on that chain's alone, and acf[k] on no lag but k.
#include "gpt_internal.h"
#include "device_util.h"

namespace gpt {

constexpr int kDgLanes = 64;       // parameters per workgroup
constexpr int kTC = 32;            // samples per time chunk
constexpr int kKB = 16;            // lags per wave, in registers
constexpr int kSB = 8;             // samples per register block
constexpr int kDgWaves = 4;        // waves per workgroup
constexpr int kKG = kKB * kDgWaves;  // lags per workgroup
static_assert(kTC % kSB == 0, "a chunk is whole register blocks");

int diag_time_chunk() { return kTC; }
int diag_lag_block() { return kKB; }
int diag_lag_group() { return kKG; }
int diag_lag_groups(int K) { return K < 1 ? 1 : (K + kKG - 1) / kKG; }

#pragma clang fp contract(off)     // nothing below fuses but the __builtin_fma of the lag products
__global__ __launch_bounds__(kDgLanes) void diag_mean_kernel(
    const double* __restrict__ x, long long P, long long cstride, int S,
    double* __restrict__ chain_mean, double* __restrict__ ebar_out, double* __restrict__ hbar_out) {
  const long long p = (long long)blockIdx.x * kDgLanes + threadIdx.x;
  const int m = blockIdx.y;
  if (p >= P) return;
  const double* f = x + p + (size_t)cstride * m;
  const int H = S / 2;
  const double x0 = f[0];
  double tot = 0.0, se = 0.0, h1 = 0.0, h2 = 0.0;
  int s = 0;
#pragma unroll 8
  for (; s < H; ++s) {
    const double v = f[(size_t)s * P];
    tot += v;
    se += v - x0;
    h1 += v - x0;
  }
  if (S & 1) {                                       // the middle sample belongs to neither half
    const double v = f[(size_t)s * P];
    tot += v;
    se += v - x0;
    ++s;
  }
#pragma unroll 8
  for (; s < S; ++s) {
    const double v = f[(size_t)s * P];
    tot += v;
    se += v - x0;
    h2 += v - x0;
  }
  const size_t o = (size_t)p + (size_t)P * m;
  chain_mean[o] = tot / S;
  ebar_out[o] = se / S;
  hbar_out[2 * o] = h1 / H;
  hbar_out[2 * o + 1] = h2 / H;
}

// macov (P, K + 1) = (Σ_m acov_m(k))/M; chain_var (P, M); hq (2, P, M) the half-chain sums of squares;
// chain_acov (P, K + 1, M) or null: the raw acov_m(k), which diag_chain_acf_kernel normalises.
__global__ __launch_bounds__(kDgLanes * kDgWaves) void diag_acov_kernel(
    const double* __restrict__ x, long long P, long long cstride, int S, int M, int K,
    const double* __restrict__ ebar, const double* __restrict__ hbar, double* __restrict__ macov,
    double* __restrict__ chain_var, double* __restrict__ hq, double* __restrict__ chain_acov) {
  __shared__ double L[kTC][kDgLanes];                // the chunk's own samples (groups past the first)
  __shared__ double R[kTC + kKG][kDgLanes];          // samples s0 + kg0 + j, j = 0 … kTC + kKG − 1
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = blockIdx.y;
  const int kg0 = g * kKG;                           // this group's lags are kg0 + 1 … kg0 + kKG
  const int off = 1 + wv * kKB;                      // this wave's first lag, relative to kg0
  const long long p = (long long)blockIdx.x * kDgLanes + lane;
  const bool live = p < P;
  const bool lag0 = g == 0 && wv == 0;
  const bool active = kg0 + off <= K;                // the wave has a lag to keep
  const int H = S / 2;
  // the rows of R in use: the chunk and a halo of the lags this group keeps
  const int nrow = kTC + min(kKG, K - kg0);
  const int send = g == 0 ? S : S - kg0 - 1;         // samples past send pair with nothing here
  const double (*left)[kDgLanes] = g == 0 ? R : L;

  double sum[kKB], sum0 = 0.0;
#pragma unroll
  for (int q = 0; q < kKB; ++q) sum[q] = 0.0;

  for (int m = 0; m < M; ++m) {
    const size_t o = (size_t)(live ? p : 0) + (size_t)P * m;
    const double* f = x + (live ? p : 0) + (size_t)cstride * m;
    const double x0 = live ? f[0] : 0.0, eb = live ? ebar[o] : 0.0;
    double d1 = 0.0, d2 = 0.0, q1 = 0.0, q2 = 0.0;
    if (lag0) { d1 = hbar[2 * o] - eb; d2 = hbar[2 * o + 1] - eb; }
    double acc[kKB], acc0 = 0.0;
#pragma unroll
    for (int q = 0; q < kKB; ++q) acc[q] = 0.0;

    for (int s0 = 0; s0 < send; s0 += kTC) {
      __syncthreads();                               // the previous chunk has been read
      for (int j = wv; j < nrow; j += kDgWaves) {
        const int t = s0 + kg0 + j;
        R[j][lane] = (live && t < S) ? (f[(size_t)t * P] - x0) - eb : 0.0;
      }
      if (g != 0)
        for (int j = wv; j < kTC; j += kDgWaves) {
          const int t = s0 + j;
          L[j][lane] = (live && t < S) ? (f[(size_t)t * P] - x0) - eb : 0.0;
        }
      __syncthreads();
      if (active) {
#pragma unroll 1
        for (int i0 = 0; i0 < kTC; i0 += kSB) {
          double l[kSB], r[kSB + kKB - 1];
#pragma unroll
          for (int i = 0; i < kSB; ++i) l[i] = left[i0 + i][lane];
#pragma unroll
          for (int j = 0; j < kSB + kKB - 1; ++j) r[j] = R[i0 + off + j][lane];
#pragma unroll
          for (int i = 0; i < kSB; ++i)
#pragma unroll
            for (int q = 0; q < kKB; ++q) acc[q] = __builtin_fma(l[i], r[i + q], acc[q]);
          if (lag0) {
#pragma unroll
            for (int i = 0; i < kSB; ++i) {
              acc0 = __builtin_fma(l[i], l[i], acc0);
              const int s = s0 + i0 + i;             // wave-uniform
              if (s < H) {
                const double e = l[i] - d1;
                q1 = __builtin_fma(e, e, q1);
              } else if (s >= S - H && s < S) {
                const double e = l[i] - d2;
                q2 = __builtin_fma(e, e, q2);
              }
            }
          }
        }
      }
    }
    if (active && live) {
#pragma unroll
      for (int q = 0; q < kKB; ++q) {
        const int k = kg0 + off + q;
        const double a = acc[q] / S;
        sum[q] += a;
        if (chain_acov && k <= K) chain_acov[(size_t)p + (size_t)P * (k + (size_t)(K + 1) * m)] = a;
      }
      if (lag0) {
        const double a = acc0 / S;
        sum0 += a;
        if (chain_acov) chain_acov[(size_t)p + (size_t)P * ((size_t)(K + 1) * m)] = a;
        chain_var[o] = a * S / (S - 1);
        hq[o] = q1;
        hq[o + (size_t)P * M] = q2;
      }
    }
  }
  if (active && live) {
#pragma unroll
    for (int q = 0; q < kKB; ++q) {
      const int k = kg0 + off + q;
      if (k <= K) macov[(size_t)p + (size_t)P * k] = sum[q] / M;
    }
    if (lag0) macov[p] = sum0 / M;
  }
}

// chain_acf (P, K + 1, M) in place: acov_m(k)/acov_m(0), lag 0 last
__global__ __launch_bounds__(kDgLanes) void diag_chain_acf_kernel(double* __restrict__ ca, long long P,
                                                                 int K) {
  const long long p = (long long)blockIdx.x * kDgLanes + threadIdx.x;
  if (p >= P) return;
  double* a = ca + p + (size_t)P * (size_t)(K + 1) * blockIdx.y;
  const double a0 = a[0];
  for (int k = K; k >= 0; --k) a[(size_t)P * k] = a[(size_t)P * k] / a0;
}

__global__ __launch_bounds__(kDgLanes) void diag_finish_kernel(
    const double* __restrict__ x, long long P, long long cstride, int S, int M, int K,
    double tau_floor, const double* __restrict__ chain_mean, const double* __restrict__ ebar,
    const double* __restrict__ hbar, const double* __restrict__ chain_var,
    const double* __restrict__ hq, const double* __restrict__ macov, double* __restrict__ mean_out,
    double* __restrict__ sd_out, double* __restrict__ rhat_out, double* __restrict__ ess_out,
    double* __restrict__ mcse_out, double* __restrict__ tau_out, int32_t* __restrict__ trunc_out,
    double* __restrict__ acf_out) {
  const long long p = (long long)blockIdx.x * kDgLanes + threadIdx.x;
  if (p >= P) return;
  const int H = S / 2;
  const size_t PM = (size_t)P * M;
  const double x00 = x[p], e00 = ebar[p], h00 = hbar[2 * (size_t)p];
  // pass 1 over the chains: the means of the means (in deviations from chain 0's)
  double sm = 0.0, sw = 0.0, se = 0.0, sh = 0.0, swh = 0.0;
  for (int m = 0; m < M; ++m) {
    const size_t o = (size_t)p + (size_t)P * m;
    const double dx = x[p + (size_t)cstride * m] - x00;
    sm += chain_mean[o];
    sw += chain_var[o];
    se += dx + (ebar[o] - e00);
    sh += dx + (hbar[2 * o] - h00);
    sh += dx + (hbar[2 * o + 1] - h00);
    swh += hq[o] / (H - 1);
    swh += hq[o + PM] / (H - 1);
  }
  const double mean = sm / M, W = sw / M, ebm = se / M, hbm = sh / (2 * M), Wh = swh / (2 * M);
  double qb = 0.0, qh = 0.0;
  for (int m = 0; m < M; ++m) {
    const size_t o = (size_t)p + (size_t)P * m;
    const double dx = x[p + (size_t)cstride * m] - x00;
    const double e = (dx + (ebar[o] - e00)) - ebm;
    qb += e * e;
    const double a = (dx + (hbar[2 * o] - h00)) - hbm, b = (dx + (hbar[2 * o + 1] - h00)) - hbm;
    qh += a * a;
    qh += b * b;
  }
  const double BS = M > 1 ? qb / (M - 1) : 0.0;      // B/S
  const double BH = qh / (2 * M - 1);                // B_h/H
  const double varp = W * (S - 1) / S + BS;
  const double sd = sqrt(varp);
  mean_out[p] = mean;
  sd_out[p] = sd;
  const double nan = __builtin_nan("");
  if (!(varp != 0.0)) {                              // a constant parameter
    rhat_out[p] = ess_out[p] = mcse_out[p] = tau_out[p] = nan;
    trunc_out[p] = 0;
    if (acf_out)
      for (int k = 0; k <= K; ++k) acf_out[(size_t)p + (size_t)P * k] = nan;
    return;
  }
  rhat_out[p] = sqrt(((double)(H - 1) / H * Wh + BH) / Wh);
  // Geyer's initial monotone sequence on the pairs (2j, 2j + 1)
  double sumP = 0.0, prev = 0.0;
  int stopped = 0;
  for (int k = 0; k <= K; k += 2) {
    const double r0 = 1.0 - (W - macov[(size_t)p + (size_t)P * k]) / varp;
    if (acf_out) acf_out[(size_t)p + (size_t)P * k] = r0;
    if (k + 1 > K) break;
    const double r1 = 1.0 - (W - macov[(size_t)p + (size_t)P * (k + 1)]) / varp;
    if (acf_out) acf_out[(size_t)p + (size_t)P * (k + 1)] = r1;
    if (stopped) {
      if (!acf_out) break;
      continue;
    }
    double Pj = r0 + r1;
    if (Pj <= 0.0) { stopped = 1; continue; }
    if (k > 0) Pj = fmin(Pj, prev);
    sumP += Pj;
    prev = Pj;
  }
  const double tau = fmax(-1.0 + 2.0 * sumP, tau_floor);
  const double ess = (double)M * S / tau;
  tau_out[p] = tau;
  ess_out[p] = ess;
  mcse_out[p] = sd / sqrt(ess);
  trunc_out[p] = !stopped;
}

size_t diag_ws_doubles(long long P, int M, int K) {
  return (size_t)P * (K + 1) + 7 * (size_t)P * M;
}

// ws: macov P·(K+1) | chain_mean P·M | chain_var P·M | ebar P·M | hbar 2·P·M | hq 2·P·M (the two
// outputs land in the caller's arrays where given).  x points at the window's first sample.
hipError_t launch_chain_diag(const double* x, long long P, long long cstride, int S, int M, int K,
                             double* ws, double* mean, double* sd, double* rhat, double* ess,
                             double* mcse, double* tau, int32_t* truncated, double* chain_mean,
                             double* chain_var, double* acf, double* chain_acf, hipStream_t st) {
  const long long ptiles = (P + kDgLanes - 1) / kDgLanes;
  const int G = diag_lag_groups(K);
  if (P < 1 || S < 4 || M < 1 || M > 65535 || K < 1 || K > S - 1 || ptiles > 0x7fffffffLL)
    return hipErrorInvalidValue;
  const size_t PM = (size_t)P * M;
  double* macov = ws;
  double* cm = chain_mean ? chain_mean : macov + (size_t)P * (K + 1);
  double* cv = chain_var ? chain_var : macov + (size_t)P * (K + 1) + PM;
  double* eb = macov + (size_t)P * (K + 1) + 2 * PM;
  double* hb = eb + PM;
  double* hq = hb + 2 * PM;
  hipLaunchKernelGGL(diag_mean_kernel, dim3((unsigned)ptiles, (unsigned)M), dim3(kDgLanes), 0, st, x,
                     P, cstride, S, cm, eb, hb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(diag_acov_kernel, dim3((unsigned)ptiles, (unsigned)G),
                     dim3(kDgLanes * kDgWaves), 0, st, x, P, cstride, S, M, K, eb, hb, macov, cv, hq,
                     chain_acf);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (chain_acf) {
    hipLaunchKernelGGL(diag_chain_acf_kernel, dim3((unsigned)ptiles, (unsigned)M), dim3(kDgLanes), 0,
                       st, chain_acf, P, K);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const double tau_floor = 1.0 / log10((double)M * (double)S);
  hipLaunchKernelGGL(diag_finish_kernel, dim3((unsigned)ptiles), dim3(kDgLanes), 0, st, x, P, cstride,
                     S, M, K, tau_floor, cm, eb, hb, cv, hq, macov, mean, sd, rhat, ess, mcse, tau,
                     truncated, acf);
  return hipGetLastError();
}

}  // namespace gpt
