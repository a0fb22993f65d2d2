// Posterior predictive of a sampled regression model from its stored predictions F (Ntest, T),
// column s at F + s·Ntest (the layout of gpt_pred_dev and nt_scores_kernel), over the window's
// S = last − first columns, in sample order, with noise variance v:
//   fmu   = (Σ_s f_s)/S                      the sum and the division of mean_sse_kernel: same bits
//   fs2   = (Σ_s ((f_s − p) − ebar)²)/S      p = the window's first f, ebar = (Σ_s (f_s − p))/S
//   ys2   = fs2 + v,  lp = −(y − fmu)²/(2 ys2) − ½ log(2π ys2)           (GPkit's moment match)
//   lpmix = −½ log(2π v) − log S − m/(2v) + log Σ_s exp((m − (y − f_s)²)/(2v)),  m = min_s (y − f_s)²
// fs2 is the two-pass variance with divisor S of the deviations from p: f_s − fmu written as
// (f_s − p) − mean(f − p).  Subtracting p first is exact where the columns agree, so equal columns
// give fs2 == 0.0 (Σ of S copies of f, divided by S, need not return f, so f_s − fmu would leave a
// rounding of fmu there), and it takes a common offset out before anything is squared.  A sum of
// squares over S: never negative, no clamp.  lpmix is the max-shifted logsumexp with the shift
// applied to the squared residuals: the nearest sample's term is exp(0) = 1, so the sum is in
// [1, S] whatever underflows.
//
// One thread per row, rows across the lanes (a wave's load of a column is 512 contiguous bytes),
// kPvRows rows per workgroup, two passes over the row's S values, neither split over threads:
// every sum above is one chain in sample order, and a row's results depend on its own S values,
// y and v alone.  The per-call sums follow class_eval_kernel: a tile's Σ lp and Σ lpmix are one
// wave_sum per wave and the waves in order, the covered rows (|y − fmu| <= z·sqrt(ys2)) are
// counted by ballot, and predictive_finish_kernel adds the tiles in tile order.  The tile size is
// fixed, so the sums depend on the rows and their order alone.
#include "gpt_internal.h"
#include "device_util.h"

namespace gpt {

constexpr int kPvRows = 256;
constexpr double kZ95 = 1.959963984540054;           // the 0.975 quantile of the standard normal

#pragma clang fp contract(off)                       // every product below is rounded before its sum
__global__ __launch_bounds__(kPvRows) void predictive_kernel(
    const double* __restrict__ F, const double* __restrict__ y, long long Ntest, int S,
    double noise_var, double* __restrict__ fmu_out, double* __restrict__ fs2_out,
    double* __restrict__ lp_out, double* __restrict__ lpmix_out, double* __restrict__ part,
    int32_t* __restrict__ part_cov) {
  __shared__ double red[2][kPvRows / 64];
  __shared__ int redc[kPvRows / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long i = (long long)blockIdx.x * kPvRows + tid;
  double lp = 0.0, lpmix = 0.0;
  int cov = 0;
  if (i < Ntest) {
    const double* f = F + i;
    const double yi = y[i], p = f[0];
    double m = 0.0, se = 0.0, dmin = INFINITY;
#pragma unroll 8
    for (int s = 0; s < S; ++s) {
      const double v = f[(size_t)s * Ntest];
      m += v;
      se += v - p;
      const double d = yi - v;
      dmin = fmin(dmin, d * d);
    }
    m /= S;
    const double ebar = se / S;
    const double inv2v = 1.0 / (2.0 * noise_var);
    double q = 0.0, es = 0.0;
#pragma unroll 8
    for (int s = 0; s < S; ++s) {
      const double v = f[(size_t)s * Ntest];
      const double e = (v - p) - ebar;
      q += e * e;
      const double d = yi - v;
      es += exp((dmin - d * d) * inv2v);
    }
    const double fs2 = q / S;
    const double ys2 = fs2 + noise_var;
    const double r = yi - m;
    lp = -(r * r) / (2.0 * ys2) - 0.5 * log(2.0 * M_PI * ys2);
    lpmix = ((-0.5 * log(2.0 * M_PI * noise_var) - log((double)S)) - dmin * inv2v) + log(es);
    cov = fabs(r) <= kZ95 * sqrt(ys2);
    if (fmu_out) fmu_out[i] = m;
    if (fs2_out) fs2_out[i] = fs2;
    if (lp_out) lp_out[i] = lp;
    if (lpmix_out) lpmix_out[i] = lpmix;
  }
  const double wl = wave_sum(lp), wm = wave_sum(lpmix);
  const int wc = __popcll(__ballot(cov));
  if (lane == 0) { red[0][wv] = wl; red[1][wv] = wm; redc[wv] = wc; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    int c = 0;
    for (int w = 0; w < kPvRows / 64; ++w) { a += red[0][w]; b += red[1][w]; c += redc[w]; }
    part[2 * (size_t)blockIdx.x] = a;
    part[2 * (size_t)blockIdx.x + 1] = b;
    part_cov[blockIdx.x] = c;
  }
}

// sums[0] = Σ lp, sums[1] = Σ lpmix, *covered = the covered rows: the tiles in tile order
__global__ void predictive_finish_kernel(const double* __restrict__ part,
                                         const int32_t* __restrict__ part_cov, long long ntiles,
                                         double* __restrict__ sums, double* __restrict__ covered) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double a = 0.0, b = 0.0;
  long long c = 0;
  for (long long k = 0; k < ntiles; ++k) {
    a += part[2 * k];
    b += part[2 * k + 1];
    c += part_cov[k];
  }
  sums[0] = a;
  sums[1] = b;
  *covered = (double)c;                              // an integer value: exact below 2^53 rows
}

size_t predictive_tiles(long long Ntest) { return (size_t)((Ntest + kPvRows - 1) / kPvRows); }

hipError_t launch_predictive(const double* F, const double* y, long long Ntest, int S,
                             double noise_var, double* fmu, double* fs2, double* lp, double* lpmix,
                             double* part, int32_t* part_cov, double* sums, double* covered,
                             hipStream_t st) {
  const size_t ntiles = predictive_tiles(Ntest);
  if (Ntest < 1 || ntiles > 0x7fffffffULL || S < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(predictive_kernel, dim3((unsigned)ntiles), dim3(kPvRows), 0, st, F, y, Ntest,
                     S, noise_var, fmu, fs2, lp, lpmix, part, part_cov);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(predictive_finish_kernel, dim3(1), dim3(64), 0, st, part, part_cov,
                     (long long)ntiles, sums, covered);
  return hipGetLastError();
}

}  // namespace gpt
