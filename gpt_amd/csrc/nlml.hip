// Gaussian marginal likelihood of the no-tensor random-Fourier-feature GP and its gradient with
// respect to [length_scale; sigma_RBF; signal_var] (GPNT_nlogmarginal / GPNT_gradnlogmarginal,
// GPT_SGLD.jl:921-962, with gradfeatureNotensor :142-177) for MI355X (gfx950).  DESIGN §6c.
//
// phi (n × N) = c·cos f, S = c·sin f, f = Zt·Xᵀ + b, Zt = Z ./ ℓ, c = sqrt(2/n)·σ_RBF;
// A = phi·phiᵀ + σ²I = L·Lᵀ, bv = phi·y, l = A⁻¹bv.  The value needs only those (tgp.hip's SYRK,
// GEMV, Cholesky and triangular solves).  The reference's gradient forms dphi/dh for every
// hyper-parameter and runs a GEMM and two n × n solves on each; here, with P = A⁻¹, e = phiᵀl − y,
// W = P·phi and T = S ∘ (W + l·eᵀ/σ²),
//   d/dℓ_k = (1/ℓ_k) Σ_j Zt[j,k]·(T·X)[j,k],   d/dσ_RBF = (n − σ² tr P − lᵀl)/σ_RBF,
//   d/dσ²  = (N−n)/(2σ²) + tr P/2 + (lᵀbv − yᵀy)/(2σ⁴) + lᵀl/(2σ²):
// one GEMM (W, never stored) whose epilogue contracts with S and X.  All fp64, no atomics, every
// sum in a fixed order.
//
// From the same factor, the model's closed-form predictive (fmu = phisᵀl, fs2 = σ²·colsum((L⁻¹phis)²),
// lp: gpt_nlml_predict), and the error of phiᵀphi against the exact kernel matrix
// (gpt_rff_kernel_error, PowerPlantDataExperiment.jl:47-97).  DESIGN §6f.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "device_util.h"
#include "exactgp.h"
#include "host_util.h"
#include "mfma_tile.h"

namespace gpt {

constexpr int kNlmlNMax = 1024;      // the blocked single-workgroup Cholesky's limit

// phi[j + n i] = c·cos(f), S[j + n i] = c·sin(f): the argument formed exactly as
// feature_notensor_kernel forms it, so phi is gpt_feature_notensor's double.  S may be null.
__global__ __launch_bounds__(256) void nlml_feature_kernel(
    const double* __restrict__ X, long long N, int D, const double* __restrict__ ls, double c,
    const double* __restrict__ Z, const double* __restrict__ b, int n, double* __restrict__ phi,
    double* __restrict__ S) {
  const long long total = (long long)n * N;
  for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < total;
       x += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(x % n);
    const long long i = x / n;
    double s = 0.0;
    for (int k = 0; k < D; ++k)
      s = __dadd_rn(s, __dmul_rn(X[i + N * k], __dmul_rn(Z[j + (long long)n * k], 1.0 / ls[k])));
    const double f = __dadd_rn(s, b[j]);
    phi[x] = c * cos(f);
    if (S) S[x] = c * sin(f);
  }
}

// e[i] = Σ_j phi[j + n i]·l[j] − y[i]: one wave per data column, lanes over j (coalesced), the
// lane sums combined in wave_sum's fixed pattern.
__global__ __launch_bounds__(256) void nlml_resid_kernel(const double* __restrict__ phi,
                                                         const double* __restrict__ l,
                                                         const double* __restrict__ y, int n,
                                                         long long N, double* __restrict__ e) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const double* col = phi + (size_t)n * i;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s = fma(col[j], l[j], s);
  s = wave_sum(s);
  if (lane == 0) e[i] = s - y[i];
}

// Xt = L⁻ᵀ (column-major n × n, Xt[c + n i] = (L⁻¹)[i, c]; the caller zeroes it first) from the
// factor chol_blk_kernel leaves: L in the lower triangle, Lᵀ in the upper one.  One workgroup per
// block of kTiRC right-hand-side columns of the identity; rows in panels of 16 from the block's
// first row down (the rows above are zero).  Per panel: the 256 threads hold one (row, column)
// entry each and subtract Σ_k L[i,k]·X[k,c] over the rows solved so far, with L[i, k..] read from
// the upper triangle (contiguous in k) through LDS in chunks of kTiKC and the solved X block kept
// in LDS; then 16 threads solve the panel's 16 × 16 triangle, a column each.
constexpr int kTiRC = 16;
constexpr int kTiKC = 128;
static size_t trinv_lds_bytes(int n) {
  const int NP = (n + 15) / 16 * 16;
  return 8 * ((size_t)NP * kTiRC + 16 * (kTiKC + 1) + 2 * 16 * 17);
}
__global__ __launch_bounds__(256) void nlml_trinv_kernel(const double* __restrict__ M, int n,
                                                         double* __restrict__ Xt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int NP = (n + 15) / 16 * 16;
  double* Xs = (double*)smem;                  // Xs[(i − c0)·16 + c]
  double* Lp = Xs + (size_t)NP * kTiRC;        // Lp[row·(kTiKC+1) + k]
  double* Tr = Lp + 16 * (kTiKC + 1);          // the panel's triangle, Tr[row·17 + col]
  double* Ac = Tr + 16 * 17;                   // right-hand sides of the triangle solve
  const int tid = threadIdx.x, il = tid & 15, cl = tid >> 4;
  const int c0 = blockIdx.x * kTiRC;
  for (int r0 = c0; r0 < NP; r0 += 16) {
    double a = (r0 + il == c0 + cl) ? 1.0 : 0.0;
    for (int kc = c0; kc < r0; kc += kTiKC) {
      const int len = min(kTiKC, r0 - kc);
      __syncthreads();
      for (int x = tid; x < 16 * len; x += 256) {
        const int ii = x / len, kk = x - ii * len, i = r0 + ii;
        Lp[ii * (kTiKC + 1) + kk] = i < n ? M[(size_t)(kc + kk) + (size_t)n * i] : 0.0;
      }
      __syncthreads();
      const double* lrow = Lp + il * (kTiKC + 1);
      const double* xcol = Xs + (size_t)(kc - c0) * kTiRC + cl;
      for (int kk = 0; kk < len; ++kk) a -= lrow[kk] * xcol[(size_t)kk * kTiRC];
    }
    {
      const int i = r0 + il, k = r0 + cl;
      Tr[il * 17 + cl] = (i < n && cl <= il) ? M[(size_t)i + (size_t)n * k] : (il == cl ? 1.0 : 0.0);
      Ac[il * 17 + cl] = a;
    }
    __syncthreads();
    if (tid < kTiRC) {
      double x[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        double s = Ac[i * 17 + tid];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= Tr[i * 17 + k] * x[k];
        x[i] = s / Tr[i * 17 + i];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) Xs[(size_t)(r0 - c0 + i) * kTiRC + tid] = x[i];
    }
    __syncthreads();
    {
      const int i = r0 + (tid >> 4), c = c0 + (tid & 15);
      if (i < n && c < n) Xt[(size_t)c + (size_t)n * i] = Xs[(size_t)(i - c0) * kTiRC + (tid & 15)];
    }
  }
}

// The SYRK writes the lower 16 × 16 tiles: mirror them (nlml_grad_kernel reads whole rows).
__global__ __launch_bounds__(256) void nlml_mirror_kernel(double* __restrict__ P, int n) {
  const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
  if (x >= (long long)n * n) return;
  const int a = (int)(x % n), c = (int)(x / n);
  if (a < c) P[x] = P[(size_t)c + (size_t)n * a];
}

// The gradient's hot path.  W = P·phi on v_mfma_f64_16x16x4f64 with K = n, never stored: a wave
// owns 32 features j (two 16-wide tiles) of one block of CB data columns and walks the block 32
// columns at a time (2 × 2 MFMA tiles).  The MFMA's first operand is phi (rows ↔ data columns i)
// and its second P (columns ↔ features j; P is symmetric, so row j is contiguous in K), so lane λ
// receives D[i = (λ>>4) + 4·reg][j = λ&15]: the sum over i of T[j,i]·X[i,k] runs inside the lane
// over reg and over the tiles of the block (g[·][k], D <= DP registers), and only the four lane
// groups λ>>4 are combined at the end (two exchange rounds).  Both operands are K-contiguous: the
// K loop is mfma_kpair_tile (mfma_tile.h).  Lanes of rows i >= N or features j >= n read row 0 and
// their T is selected to an exact zero.  part[(cb·n + j)·D + k] = Σ_{i in block cb} T[j,i]·X[i,k].
template <bool V2, int DP>
__global__ __launch_bounds__(256) void nlml_grad_kernel(
    const double* __restrict__ P, const double* __restrict__ phi, const double* __restrict__ S,
    const double* __restrict__ l, const double* __restrict__ e, const double* __restrict__ X, int n,
    long long N, int D, int CB, int ncb, double inv_s2, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wv = uni(threadIdx.x >> 6), kl = lane >> 4, li = lane & 15;
  const int npair = ((n + 15) / 16 + 1) / 2;
  const long long task = (long long)blockIdx.x * 4 + wv;
  if (task >= (long long)ncb * npair) return;
  const int cb = (int)(task / npair), jp = (int)(task - (long long)cb * npair);
  const long long i_begin = (long long)cb * CB, i_end = min(N, i_begin + CB);
  const int j0 = jp * 32;
  const double* pb[2];
  double lj[2];
  bool jok[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = j0 + 16 * u + li;
    jok[u] = j < n;
    pb[u] = P + (size_t)n * (jok[u] ? j : 0);
    lj[u] = l[jok[u] ? j : 0];
  }
  double g[2][DP];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int k = 0; k < DP; ++k) g[u][k] = 0.0;

  for (long long it = i_begin; it < i_end; it += 32) {
    const double* pa[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const long long i = it + 16 * t + li;
      pa[t] = phi + (size_t)n * (i < i_end ? i : i_begin);
    }
    d4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
    mfma_kpair_tile<V2, 2, 2>(pa, pb, n, n, kl, acc);
    // epilogue in the MFMA output layout: acc[t][u][reg] = W[j0 + 16u + li, it + 16t + kl + 4reg]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const long long i = it + 16 * t + kl + 4 * reg;
        const bool iok = i < i_end;
        const long long ic = iok ? i : i_begin;
        const double ei = e[ic] * inv_s2;
        double xv[DP];
#pragma unroll
        for (int k = 0; k < DP; ++k) xv[k] = k < D ? X[ic + N * k] : 0.0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int jc = jok[u] ? j0 + 16 * u + li : 0;
          const double sv = S[(size_t)jc + (size_t)n * ic];
          const double tv = (iok && jok[u]) ? sv * (acc[t][u][reg] + lj[u] * ei) : 0.0;
#pragma unroll
          for (int k = 0; k < DP; ++k) g[u][k] = fma(tv, xv[k], g[u][k]);
        }
      }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      double v = self_sum<32>(g[u][k], lane);
      v = self_sum<16>(v, lane);
      if (kl == 0 && jok[u] && k < D) part[((size_t)cb * n + (j0 + 16 * u + li)) * D + k] = v;
    }
}

// gl[k] = (1/ℓ_k) Σ_j Zt[j,k]·Σ_cb part[cb][j][k]: the column blocks in block order, then the
// features over the workgroup (blk_sum's fixed pattern).  One workgroup per k.
__global__ __launch_bounds__(kNT) void nlml_finish_kernel(const double* __restrict__ part, int ncb,
                                                          const double* __restrict__ Z,
                                                          const double* __restrict__ ls, int n,
                                                          int D, double* __restrict__ gl) {
  __shared__ double red[kNW];
  const int k = blockIdx.x;
  const double inv = 1.0 / ls[k];
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += kNT) {
    double gsum = 0.0;
    for (int cb = 0; cb < ncb; ++cb) gsum += part[((size_t)cb * n + j) * D + k];
    s = fma(__dmul_rn(Z[j + (size_t)n * k], inv), gsum, s);
  }
  const double tot = blk_sum(s, red);
  if (threadIdx.x == 0) gl[k] = tot / ls[k];
}

// out = {Σ log diag(L), yᵀy, bvᵀl, lᵀl, tr P (0 when P is null)}
__global__ __launch_bounds__(kNT) void nlml_scalars_kernel(const double* __restrict__ M,
                                                           const double* __restrict__ P,
                                                           const double* __restrict__ y,
                                                           const double* __restrict__ bv,
                                                           const double* __restrict__ l, int n,
                                                           long long N, double* __restrict__ out) {
  __shared__ double red[kNW];
  double ld = 0.0, yy = 0.0, bl = 0.0, ll = 0.0, tp = 0.0;
  for (int j = threadIdx.x; j < n; j += kNT) {
    ld += log(M[(size_t)j + (size_t)n * j]);
    bl = fma(bv[j], l[j], bl);
    ll = fma(l[j], l[j], ll);
    if (P) tp += P[(size_t)j + (size_t)n * j];
  }
  for (long long i = threadIdx.x; i < N; i += kNT) yy = fma(y[i], y[i], yy);
  const double a = blk_sum(ld, red), b = blk_sum(yy, red), c = blk_sum(bl, red),
               d = blk_sum(ll, red), f = blk_sum(tp, red);
  if (threadIdx.x == 0) { out[0] = a; out[1] = b; out[2] = c; out[3] = d; out[4] = f; }
}

template <bool V2>
static hipError_t launch_grad(int D, unsigned grid, hipStream_t st, const double* P,
                              const double* phi, const double* S, const double* l, const double* e,
                              const double* X, int n, long long N, int CB, int ncb, double inv_s2,
                              double* part) {
#define NLML_GRAD(DP)                                                                          \
  hipLaunchKernelGGL((nlml_grad_kernel<V2, DP>), dim3(grid), dim3(256), 0, st, P, phi, S, l, e, X, \
                     n, N, D, CB, ncb, inv_s2, part)
  if (D <= 1) NLML_GRAD(1);
  else if (D <= 2) NLML_GRAD(2);
  else if (D <= 4) NLML_GRAD(4);
  else if (D <= 8) NLML_GRAD(8);
  else NLML_GRAD(16);
#undef NLML_GRAD
  return hipGetLastError();
}

// ---------------------------------------------------------- closed-form predictive
// fmu[i] = Σ_j phis[j + n i]·l[j]: nlml_resid_kernel's wave per test column.
__global__ __launch_bounds__(256) void nlml_pmean_kernel(const double* __restrict__ phis,
                                                         const double* __restrict__ l, int n,
                                                         int nc, double* __restrict__ fmu) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nc) return;
  const double* col = phis + (size_t)n * i;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s = fma(col[j], l[j], s);
  s = wave_sum(s);
  if (lane == 0) fmu[i] = s;
}

// fs2[i] = σ²·Σ_r V[r,i]², V = L⁻¹·phis on v_mfma_f64_16x16x4f64, never stored.  A workgroup owns
// 32 test columns; its four waves take the 32-row tiles of L⁻¹ round robin (tile rt to wave
// rt mod 4, which evens out the triangle).  The MFMA's first operand is L⁻¹ (rows ↔ features r;
// row r is Xt + n·r, contiguous in K, and zero past k = r, so the K loop of tile rt stops at
// kend = min(n, 32 rt + 32)) and its second phis (columns ↔ test columns i, contiguous in K): lane
// λ receives V[r = (λ>>4) + 4·reg][i = λ&15].  The K loop is mfma_kpair_tile (mfma_tile.h) up to
// kend.  The squares are summed in a fixed order: in the lane over reg, the two row
// halves and the wave's tiles, then over the four lane groups λ>>4 (two exchange rounds), then
// over the waves in wave order through LDS.  A column's sum depends on n alone: not on the chunk,
// on nc or on its place in the tile.  Rows r >= n read row 0 and are selected to an exact zero;
// columns i >= nc read column 0 and are not written.  lp (optional) needs fmu and ytest.
template <bool V2>
__global__ __launch_bounds__(256) void nlml_pvar_kernel(
    const double* __restrict__ Xt, const double* __restrict__ phis, int n, int nc, double s2,
    const double* __restrict__ fmu, const double* __restrict__ ytest, double* __restrict__ fs2,
    double* __restrict__ lp) {
  __shared__ double red[4][32];
  const int lane = threadIdx.x & 63, wv = uni(threadIdx.x >> 6), kl = lane >> 4, li = lane & 15;
  const int i0 = blockIdx.x * 32;
  const int nrt = (n + 31) / 32;
  const double* pb[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = i0 + 16 * u + li;
    pb[u] = phis + (size_t)n * (i < nc ? i : 0);
  }
  double ss[2] = {0.0, 0.0};
  for (int rt = wv; rt < nrt; rt += 4) {
    const int r0 = 32 * rt;
    const int kend = min(n, r0 + 32);
    const double* pa[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int r = r0 + 16 * t + li;
      pa[t] = Xt + (size_t)n * (r < n ? r : 0);
    }
    d4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
    mfma_kpair_tile<V2, 2, 2>(pa, pb, n, kend, kl, acc);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const bool rok = r0 + 16 * t + kl + 4 * reg < n;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const double v = rok ? acc[t][u][reg] : 0.0;
          ss[u] = fma(v, v, ss[u]);
        }
      }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    double v = self_sum<32>(ss[u], lane);
    v = self_sum<16>(v, lane);
    if (kl == 0) red[wv][16 * u + li] = v;
  }
  __syncthreads();
  const int i = i0 + (int)threadIdx.x;
  if (threadIdx.x < 32 && i < nc) {
    const double var = s2 * (((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) +
                             red[3][threadIdx.x]);
    fs2[i] = var;
    if (lp) {
      const double ys2 = var + s2, d = ytest[i] - fmu[i];
      lp[i] = -(d * d) / (2.0 * ys2) - 0.5 * log(2.0 * M_PI * ys2);
    }
  }
}

// ------------------------------------------------------ kernel approximation error
// ‖K − K_rff‖_F, ‖K‖_F and max|K − K_rff| over all N² entries, K the squared-exponential kernel
// matrix (exactgp.hip's covariance, no noise term) and K_rff = phiᵀphi, neither ever stored.  One
// workgroup per lower 64 × 64 tile t = bi(bi+1)/2 + bj (bi >= bj); wave w owns the 32 × 32
// sub-tile (w>>1, w&1) as 2 × 2 MFMA 16×16×4 f64 accumulators, K loop over n.  Both operands are
// columns of phi (contiguous in K): the first the rows i, the second the columns j, so lane λ
// receives K_rff[i = (λ>>4) + 4·reg][j = λ&15]; the K loop is mfma_kpair_tile (mfma_tile.h), the
// tile index tri_pair.  Epilogue: the tile's X rows and columns and 1/ℓ are staged in LDS; every
// accumulator entry forms k(x_i, x_j) as exactgp.hip's egp_cov does, ((x_ik − x_jk)·(1/ℓ_k))² summed
// in k order and the device exp (dividing the rows by ℓ first would lose the difference's low
// digits at a small ℓ), and adds d², k² and max|d| in the lane (entries with i >= N or j >= N are selected to an exact zero).  Diagonal tiles are
// computed in full and count once, the others count twice.  Lane -> wave_sum / wave_max -> the
// waves in wave order -> part[3 t + {0, 1, 2}]; kerr_finish_kernel adds the tiles in tile order.
constexpr int kKerrTile = 64;
constexpr int kKerrLd = kDMax + 1;     // LDS row stride of the staged inputs

template <bool V2>
__global__ __launch_bounds__(256) void kerr_tile_kernel(const double* __restrict__ phi,
                                                        const double* __restrict__ X,
                                                        const double* __restrict__ ls, int n,
                                                        int N, int D, double sig2,
                                                        double* __restrict__ part) {
  __shared__ double xs[2][kKerrTile * kKerrLd];
  __shared__ double invl[kDMax];
  __shared__ double red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6), kl = lane >> 4, li = lane & 15;
  int bi, bj;
  tri_pair((long long)blockIdx.x, bi, bj);
  for (int x = tid; x < 2 * kKerrTile * D; x += 256) {
    const int side = x / (kKerrTile * D), rem = x - side * kKerrTile * D;
    const int k = rem / kKerrTile, r = rem - k * kKerrTile;
    const int row = min((side ? bj : bi) * kKerrTile + r, N - 1);
    xs[side][r * kKerrLd + k] = X[row + (size_t)N * k];
  }
  if (tid < D) invl[tid] = 1.0 / ls[tid];
  const int i0 = bi * kKerrTile + 32 * (wv >> 1), j0 = bj * kKerrTile + 32 * (wv & 1);
  const double *pa[2], *pb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int i = i0 + 16 * t + li, j = j0 + 16 * t + li;
    pa[t] = phi + (size_t)n * (i < N ? i : 0);
    pb[t] = phi + (size_t)n * (j < N ? j : 0);
  }
  d4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
  mfma_kpair_tile<V2, 2, 2>(pa, pb, n, n, kl, acc);
  __syncthreads();                       // the staged inputs
  double sd = 0.0, sk = 0.0, mx = 0.0;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int il = 32 * (wv >> 1) + 16 * t + kl + 4 * reg;      // row within the tile
      const double* xi = xs[0] + il * kKerrLd;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int jl = 32 * (wv & 1) + 16 * u + li;
        const double* xj = xs[1] + jl * kKerrLd;
        double s = 0.0;
        for (int k = 0; k < D; ++k) {
          const double d = (xi[k] - xj[k]) * invl[k];
          s = fma(d, d, s);
        }
        const bool ok = bi * kKerrTile + il < N && bj * kKerrTile + jl < N;
        const double kv = ok ? sig2 * exp(-0.5 * s) : 0.0;
        const double dv = ok ? kv - acc[t][u][reg] : 0.0;
        sd = fma(dv, dv, sd);
        sk = fma(kv, kv, sk);
        mx = fmax(mx, fabs(dv));
      }
    }
  sd = wave_sum(sd);
  sk = wave_sum(sk);
  mx = wave_max(mx);
  if (lane == 0) { red[wv][0] = sd; red[wv][1] = sk; red[wv][2] = mx; }
  __syncthreads();
  if (tid == 0) {
    const double w = bi == bj ? 1.0 : 2.0;
    double* out = part + 3 * (size_t)blockIdx.x;
    out[0] = w * (((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]);
    out[1] = w * (((red[0][1] + red[1][1]) + red[2][1]) + red[3][1]);
    out[2] = fmax(fmax(red[0][2], red[1][2]), fmax(red[2][2], red[3][2]));
  }
}

// out = {sqrt Σ_t part[3t], sqrt Σ_t part[3t+1], max_t part[3t+2]}: lanes 0, 1, 2 take one
// quantity each and walk the tiles in tile order.
__global__ __launch_bounds__(64) void kerr_finish_kernel(const double* __restrict__ part,
                                                         long long ntiles,
                                                         double* __restrict__ out) {
  const int q = threadIdx.x;
  if (q >= 3) return;
  double a = 0.0;
  for (long long t = 0; t < ntiles; ++t) {
    const double v = part[3 * t + q];
    a = q == 2 ? fmax(a, v) : a + v;
  }
  out[q] = q == 2 ? a : sqrt(a);
}

}  // namespace gpt

using namespace gpt;

// ------------------------------------------------------------------------------ host side
#include "gp_handle.h"

struct gpt_nlml {
  int n = 0, D = 0, CB = 0, ncb = 0;
  long long N = 0;
  double *X = nullptr, *y = nullptr, *Z = nullptr, *b = nullptr, *ls = nullptr, *phi = nullptr,
         *S = nullptr, *A = nullptr, *Xt = nullptr, *P = nullptr, *bv = nullptr, *l = nullptr,
         *e = nullptr, *part = nullptr, *gl = nullptr, *scal = nullptr;
  int32_t* status = nullptr;
  bool have_features = false, have_sin = false;
  // gpt_nlml_predict: A holds the factor of the hyper-parameters of `factor`, Xt its L⁻ᵀ
  // (have_xt); phis is the test chunk's features, grown on demand
  FactorKey factor;
  bool have_xt = false;
  GrowBlock phis;
  DevSet mem;
  PhaseMarks marks;                   // gpt_nlml_eval_timed's
};

static bool nlml_dims_ok(const void* X, int64_t N, int64_t D, const void* y, const void* Z,
                         const void* b, int64_t n) {
  if (!X || !y || !Z || !b) { set_error("nlml: null input array"); return false; }
  if (n < 1 || n > kNlmlNMax) { set_error("nlml: n must be in 1..1024"); return false; }
  if (N < 1 || N > (1LL << 31) - 1) { set_error("nlml: N must be in 1..2^31-1"); return false; }
  if (D < 1 || D > kDMax) { set_error("nlml: D must be in 1..16"); return false; }
  return true;
}

static bool nlml_hyper_ok(const double* hyper, int64_t Lh, int64_t D) {
  return hyper_ok("nlml", hyper, Lh, D, 2);
}

// column block of the gradient GEMM: the largest of 256 .. 32 columns that still gives 256
// workgroups (a function of the shape alone, so that equal shapes sum in the same order)
static int nlml_col_block(int n, long long N) {
  const long long npair = ((n + 15) / 16 + 1) / 2;
  for (int cb = 256; cb > 32; cb /= 2)
    if (((N + cb - 1) / cb) * npair >= 4 * 256) return cb;
  return 32;
}

extern "C" int gpt_nlml_create(const double* X, int64_t N, int64_t D, const double* y,
                               const double* Z, const double* b, int64_t n, gpt_nlml** out) {
  if (!out) { set_error("nlml: null handle pointer"); return GPT_ERR_BAD_DIMS; }
  *out = nullptr;
  if (!nlml_dims_ok(X, N, D, y, Z, b, n)) return GPT_ERR_BAD_DIMS;
  std::unique_ptr<gpt_nlml> h(new gpt_nlml);
  h->n = (int)n; h->D = (int)D; h->N = N;
  h->CB = nlml_col_block((int)n, N);
  h->ncb = (int)((N + h->CB - 1) / h->CB);
  DevSet& M = h->mem;
  const size_t nN = (size_t)n * N, nn = (size_t)n * n;
  GPT_HIPCHK(M.upload(&h->X, X, (size_t)N * D));
  GPT_HIPCHK(M.upload(&h->y, y, (size_t)N));
  GPT_HIPCHK(M.upload(&h->Z, Z, (size_t)n * D));
  GPT_HIPCHK(M.upload(&h->b, b, (size_t)n));
  GPT_HIPCHK(M.alloc(&h->ls, (size_t)D));
  GPT_HIPCHK(M.alloc(&h->phi, nN));
  GPT_HIPCHK(M.alloc(&h->S, nN));
  GPT_HIPCHK(M.alloc(&h->A, nn));
  GPT_HIPCHK(M.alloc(&h->Xt, nn));
  GPT_HIPCHK(M.alloc(&h->P, nn));
  GPT_HIPCHK(M.alloc(&h->bv, (size_t)n));
  GPT_HIPCHK(M.alloc(&h->l, (size_t)n));
  GPT_HIPCHK(M.alloc(&h->e, (size_t)N));
  GPT_HIPCHK(M.alloc(&h->part, (size_t)h->ncb * n * D));
  GPT_HIPCHK(M.alloc(&h->gl, (size_t)D));
  GPT_HIPCHK(M.alloc(&h->scal, 8));
  GPT_HIPCHK(M.alloc(&h->status, 4));
  *out = h.release();
  return GPT_OK;
}

extern "C" int gpt_nlml_destroy(gpt_nlml* h) { return destroy_handle(h); }

// Xt := L⁻ᵀ of the factor in A
static int nlml_build_xt(gpt_nlml* h, hipStream_t st) {
  const int n = h->n;
  GPT_HIPCHK(hipMemsetAsync(h->Xt, 0, 8 * (size_t)n * n, st));
  GPT_HIPCHK(launch_big_lds<nlml_trinv_kernel>(kMaxLds, dim3((n + kTiRC - 1) / kTiRC), dim3(256),
                                               trinv_lds_bytes(n), st, h->A, n, h->Xt));
  return GPT_OK;
}

// phase_ms (kNlmlPhases, optional): device-event times of features, SYRK, GEMV, Cholesky, the two
// triangular solves, L⁻ᵀ, P (SYRK + mirror), e, the gradient GEMM, its finish, the scalars.
constexpr int kNlmlPhases = 11;
static int nlml_eval_impl(gpt_nlml* h, const double* hyper, int64_t Lh, int32_t want_grad,
                          double* nlml, double* grad, double* theta_mean, double* phase_ms) {
  if (!h || !nlml || (want_grad && !grad)) {
    set_error("nlml: null handle or output"); return GPT_ERR_BAD_DIMS;
  }
  if (!nlml_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  const int n = h->n, D = h->D;
  const long long N = h->N;
  hipStream_t st = nullptr;
  GPT_HIPCHK(h->marks.begin(phase_ms != nullptr, kNlmlPhases));
  auto mark = [&]() { h->marks.mark(st); };
  double lsv[kDMax];
  length_scales(hyper, Lh, D, 2, lsv);
  const double sigma = hyper[Lh - 2], s2 = hyper[Lh - 1];
  const double c = std::sqrt(2.0 / (double)n) * sigma;
  GPT_HIPCHK(hipMemcpyAsync(h->ls, lsv, 8 * (size_t)D, hipMemcpyHostToDevice, st));
  GPT_HIPCHK(hipMemsetAsync(h->status, 0, 16, st));
  h->have_features = h->have_sin = false;
  h->factor.clear();
  h->have_xt = false;
  mark();
  {
    const long long total = (long long)n * N;
    const int blocks = (int)std::min((total + 255) / 256, (long long)256 * 16);
    hipLaunchKernelGGL(nlml_feature_kernel, dim3(blocks), dim3(256), 0, st, h->X, N, D, h->ls, c,
                       h->Z, h->b, n, h->phi, want_grad ? h->S : nullptr);
    GPT_HIPCHK(hipGetLastError());
  }
  mark();
  GPT_HIPCHK(dense_syrk(h->phi, n, N, 1.0, s2, h->A, st));
  mark();
  GPT_HIPCHK(dense_gemv(h->phi, n, N, h->y, 1.0, h->bv, st));
  mark();
  dense_chol(h->A, n, h->status, st);
  mark();
  GPT_HIPCHK(hipMemcpyAsync(h->l, h->bv, 8 * (size_t)n, hipMemcpyDeviceToDevice, st));
  dense_trsv(h->A, n, h->l, 0, st);
  dense_trsv(h->A, n, h->l, 1, st);
  GPT_HIPCHK(hipGetLastError());
  mark();
  if (want_grad) {
    GPT_TRY(nlml_build_xt(h, st));
    mark();
    GPT_HIPCHK(dense_syrk(h->Xt, n, n, 1.0, 0.0, h->P, st));
    hipLaunchKernelGGL(nlml_mirror_kernel, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256),
                       0, st, h->P, n);
    mark();
    hipLaunchKernelGGL(nlml_resid_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, h->phi,
                       h->l, h->y, n, N, h->e);
    GPT_HIPCHK(hipGetLastError());
    mark();
    const long long npair = ((n + 15) / 16 + 1) / 2;
    const unsigned grid = (unsigned)((npair * h->ncb + 3) / 4);
    GPT_HIPCHK((n % 2 == 0)
              ? launch_grad<true>(D, grid, st, h->P, h->phi, h->S, h->l, h->e, h->X, n, N, h->CB,
                                  h->ncb, 1.0 / s2, h->part)
              : launch_grad<false>(D, grid, st, h->P, h->phi, h->S, h->l, h->e, h->X, n, N, h->CB,
                                   h->ncb, 1.0 / s2, h->part));
    mark();
    hipLaunchKernelGGL(nlml_finish_kernel, dim3(D), dim3(kNT), 0, st, h->part, h->ncb, h->Z, h->ls,
                       n, D, h->gl);
    mark();
  } else {
    for (int q = 0; q < 5; ++q) mark();
  }
  hipLaunchKernelGGL(nlml_scalars_kernel, dim3(1), dim3(kNT), 0, st, h->A,
                     want_grad ? h->P : nullptr, h->y, h->bv, h->l, n, N, h->scal);
  GPT_HIPCHK(hipGetLastError());
  mark();
  double sc[5], gl[kDMax];
  int32_t bad = 0;
  std::vector<double> lh(n);
  GPT_HIPCHK(hipMemcpyAsync(sc, h->scal, 8 * 5, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipMemcpyAsync(&bad, h->status, 4, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipMemcpyAsync(lh.data(), h->l, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
  if (want_grad) GPT_HIPCHK(hipMemcpyAsync(gl, h->gl, 8 * (size_t)D, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipStreamSynchronize(st));
  GPT_HIPCHK(h->marks.read(phase_ms));
  h->have_features = true;
  h->have_sin = want_grad != 0;
  if (bad) {
    nan_fill(nlml, 1);
    if (want_grad) nan_fill(grad, Lh);
    nan_fill(theta_mean, n);
    set_error("nlml: phi*phi' + signal_var*I is not positive definite (PosDefException)");
    return GPT_ERR_NOT_SPD;
  }
  const double logdet = sc[0], yy = sc[1], bl = sc[2], ll = sc[3], trP = sc[4];
  const double dN = (double)N, dn = (double)n;
  *nlml = (dN - dn) / 2 * std::log(s2) + logdet + (yy - bl) / (2 * s2) +
          dN / 2 * std::log(2 * M_PI);
  if (want_grad) {
    fold_ls_grad(gl, D, Lh, 2, grad);
    grad[Lh - 2] = (dn - s2 * trP) / sigma - ll / sigma;
    grad[Lh - 1] = (dN - dn) / (2 * s2) + trP / 2 + (bl - yy) / (2 * s2 * s2) + ll / (2 * s2);
  }
  if (theta_mean) std::memcpy(theta_mean, lh.data(), 8 * (size_t)n);
  h->factor.set(hyper, Lh);
  h->have_xt = want_grad != 0;
  return GPT_OK;
}

// The factor of hyper in A: the resident one when it is that of these bits, else an evaluation
// without gradient.
static int nlml_ensure_factor(gpt_nlml* h, const double* hyper, int64_t Lh) {
  if (h->factor.matches(hyper, Lh)) return GPT_OK;
  double val = 0.0;
  return nlml_eval_impl(h, hyper, Lh, 0, &val, nullptr, nullptr, nullptr);
}

static int nlml_ensure_xt(gpt_nlml* h, hipStream_t st) {
  if (!h->have_xt) GPT_TRY(nlml_build_xt(h, st));
  h->have_xt = true;
  return GPT_OK;
}

// The one-shot forms: create, body on the fresh handle, destroy.
template <class Body>
static int nlml_one_shot(const double* X, int64_t N, int64_t D, const double* y, const double* Z,
                         const double* b, int64_t n, Body&& body) {
  return one_shot<gpt_nlml>([&](gpt_nlml** h) { return gpt_nlml_create(X, N, D, y, Z, b, n, h); },
                            body);
}

extern "C" int gpt_nlml_eval(gpt_nlml* h, const double* hyper, int64_t Lh, int32_t want_grad,
                             double* nlml, double* grad, double* theta_mean) {
  return nlml_eval_impl(h, hyper, Lh, want_grad, nlml, grad, theta_mean, nullptr);
}

extern "C" int gpt_nlml_eval_timed(gpt_nlml* h, const double* hyper, int64_t Lh, int32_t want_grad,
                                   double* nlml, double* grad, double* phase_ms) {
  if (!phase_ms) { set_error("nlml: null phase_ms"); return GPT_ERR_BAD_DIMS; }
  return nlml_eval_impl(h, hyper, Lh, want_grad, nlml, grad, nullptr, phase_ms);
}

extern "C" int gpt_nlml_features(gpt_nlml* h, double* phi_out, double* sin_out) {
  if (!h || (!phi_out && !sin_out)) { set_error("nlml: null handle or output"); return GPT_ERR_BAD_DIMS; }
  if (!h->have_features || (sin_out && !h->have_sin)) {
    set_error("nlml: no evaluation yet (sin_out needs one with want_grad)");
    return GPT_ERR_BAD_DIMS;
  }
  const size_t bytes = 8 * (size_t)h->n * h->N;
  if (phi_out) GPT_HIPCHK(hipMemcpy(phi_out, h->phi, bytes, hipMemcpyDeviceToHost));
  if (sin_out) GPT_HIPCHK(hipMemcpy(sin_out, h->S, bytes, hipMemcpyDeviceToHost));
  return GPT_OK;
}

extern "C" int gpt_gpnt_nlogmarginal(const double* X, int64_t N, int64_t D, const double* y,
                                     const double* Z, const double* b, int64_t n,
                                     const double* hyper, int64_t Lh, int64_t want_grad,
                                     double* nlml_out, double* grad_out) {
  if (!nlml_dims_ok(X, N, D, y, Z, b, n) || !nlml_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  if (!nlml_out || (want_grad && !grad_out)) {
    set_error("nlml: null output"); return GPT_ERR_BAD_DIMS;
  }
  return nlml_one_shot(X, N, D, y, Z, b, n, [&](gpt_nlml* h) {
    return gpt_nlml_eval(h, hyper, Lh, want_grad ? 1 : 0, nlml_out, grad_out, nullptr);
  });
}

// ------------------------------------------------------------------ closed-form predictive
// gpt_rff_last_timing of this thread: the kernel error's features and its tile pass, the
// prediction's chunks (uploads of the chunks' rows included)
static thread_local double g_rff_ms[3] = {0.0, 0.0, 0.0};

extern "C" int gpt_rff_last_timing(double* ms, int32_t len) {
  if (!ms || len < 0) { set_error("gpt_rff_last_timing: bad output"); return GPT_ERR_BAD_DIMS; }
  for (int32_t x = 0; x < len; ++x) ms[x] = x < 3 ? g_rff_ms[x] : 0.0;
  return GPT_OK;
}

constexpr int kNlmlChunk = 4096;       // test columns per chunk when the caller passes 0, and at most

extern "C" int gpt_nlml_predict(gpt_nlml* h, const double* hyper, int64_t Lh, const double* Xtest,
                                int64_t Ntest, const double* ytest, int64_t chunk, double* fmu,
                                double* fs2, double* lp) {
  if (!h) { set_error("nlml: null handle"); return GPT_ERR_BAD_DIMS; }
  if (!nlml_hyper_ok(hyper, Lh, h->D) ||
      !test_args_ok("nlml", Xtest, Ntest, ytest, chunk, fmu, fs2, lp))
    return GPT_ERR_BAD_DIMS;
  const int n = h->n, D = h->D;
  const int rc = nlml_ensure_factor(h, hyper, Lh);
  if (rc != GPT_OK) {
    nan_fill(fmu, Ntest);
    nan_fill(fs2, Ntest);
    nan_fill(lp, Ntest);
    return rc;
  }
  hipStream_t st = nullptr;
  GPT_TRY(nlml_ensure_xt(h, st));
  const int cw = (int)std::min<int64_t>(chunk == 0 ? kNlmlChunk : std::min<int64_t>(chunk, kNlmlChunk),
                                        Ntest);
  GPT_HIPCHK(h->phis.reserve((size_t)n, (size_t)cw));
  DevMem xmem;                                              // the chunk's rows of Xtest
  TestBuffers T;
  GPT_HIPCHK(xmem.alloc<double>((size_t)cw * D));
  GPT_HIPCHK(T.alloc((size_t)Ntest, lp != nullptr));
  if (lp) GPT_HIPCHK(hipMemcpy(T.y, ytest, 8 * (size_t)Ntest, hipMemcpyHostToDevice));
  double *dX = xmem.as<double>(), *dy = T.y, *dmu = T.mu, *dv = T.v, *dlp = T.lp;
  const double sigma = hyper[Lh - 2], s2 = hyper[Lh - 1];
  const double c = std::sqrt(2.0 / (double)n) * sigma;      // h->ls holds the factor's length scales
  EventTimer tm(&g_rff_ms[2], st);
  for (int64_t c0 = 0; c0 < Ntest; c0 += cw) {
    const int nc = (int)std::min<int64_t>(cw, Ntest - c0);
    // the chunk's rows of Xtest (Ntest, D) as a dense (nc, D) block
    GPT_HIPCHK(hipMemcpy2DAsync(dX, 8 * (size_t)nc, Xtest + c0, 8 * (size_t)Ntest, 8 * (size_t)nc,
                                (size_t)D, hipMemcpyHostToDevice, st));
    const long long total = (long long)n * nc;
    hipLaunchKernelGGL(nlml_feature_kernel, dim3((unsigned)std::min((total + 255) / 256, 4096LL)),
                       dim3(256), 0, st, dX, (long long)nc, D, h->ls, c, h->Z, h->b, n, h->phis.p,
                       (double*)nullptr);
    hipLaunchKernelGGL(nlml_pmean_kernel, dim3((nc + 3) / 4), dim3(256), 0, st, h->phis.p, h->l, n,
                       nc, dmu + c0);
    if (n % 2 == 0)
      hipLaunchKernelGGL(nlml_pvar_kernel<true>, dim3((nc + 31) / 32), dim3(256), 0, st, h->Xt,
                         h->phis.p, n, nc, s2, dmu + c0, lp ? dy + c0 : (const double*)nullptr,
                         dv + c0, lp ? dlp + c0 : (double*)nullptr);
    else
      hipLaunchKernelGGL(nlml_pvar_kernel<false>, dim3((nc + 31) / 32), dim3(256), 0, st, h->Xt,
                         h->phis.p, n, nc, s2, dmu + c0, lp ? dy + c0 : (const double*)nullptr,
                         dv + c0, lp ? dlp + c0 : (double*)nullptr);
    GPT_HIPCHK(hipGetLastError());
  }
  tm.stop();
  GPT_HIPCHK(T.download(fmu, fs2, lp, st));
  GPT_HIPCHK(hipStreamSynchronize(st));
  return GPT_OK;
}

// Exact draws from θ | y ~ N(l, σ²A⁻¹) (GPNT_nlogmarginal's model, GPT_SGLD.jl:921-933):
// theta (n, S) = l·1ᵀ + σ·L⁻ᵀ·Z on the factor and the Xt = L⁻ᵀ that gpt_nlml_predict keeps.
extern "C" int gpt_nlml_draw_theta(gpt_nlml* h, const double* hyper, int64_t Lh, int64_t S,
                                   uint64_t seed, const double* Zin, double* theta, double* Zout) {
  if (S < 1 || S > kGpdSMax) { set_error("nlml draw: S must be in 1..4096"); return GPT_ERR_BAD_DIMS; }
  if (!h || !theta) { set_error("nlml draw: null handle or output"); return GPT_ERR_BAD_DIMS; }
  if (!nlml_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  const int n = h->n;
  const size_t nS = (size_t)n * S;
  const int rc = nlml_ensure_factor(h, hyper, Lh);
  if (rc != GPT_OK) {
    nan_fill(theta, (int64_t)nS);
    nan_fill(Zout, (int64_t)nS);
    return rc;
  }
  hipStream_t st = nullptr;
  DevSet tmp;
  double *dZ = nullptr, *dT = nullptr;
  GPT_HIPCHK(tmp.alloc(&dZ, nS));
  GPT_HIPCHK(tmp.alloc(&dT, nS));
  GpdTimer tm(st);
  GPT_HIPCHK(gpd_normals(dZ, n, (int)S, seed, kGpdTheta, Zin, st));
  tm.mark(0);
  GPT_TRY(nlml_ensure_xt(h, st));
  tm.mark(2);
  GPT_HIPCHK(gpd_trimm(h->Xt, (size_t)n, n, true, dZ, (int)S, h->l, std::sqrt(hyper[Lh - 1]), dT, st));
  tm.mark(5);
  GPT_HIPCHK(hipMemcpyAsync(theta, dT, 8 * nS, hipMemcpyDeviceToHost, st));
  if (Zout) GPT_HIPCHK(hipMemcpyAsync(Zout, dZ, 8 * nS, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipStreamSynchronize(st));
  tm.read();
  return GPT_OK;
}

// One-shot form: create, gpt_nlml_draw_theta, destroy.
extern "C" int gpt_gpnt_draw_theta(const double* X, int64_t N, int64_t D, const double* y,
                                   const double* Z, const double* b, int64_t n,
                                   const double* hyper, int64_t Lh, int64_t S, uint64_t seed,
                                   const double* Zin, double* theta) {
  if (!nlml_dims_ok(X, N, D, y, Z, b, n) || !nlml_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  if (S < 1 || S > kGpdSMax) { set_error("nlml draw: S must be in 1..4096"); return GPT_ERR_BAD_DIMS; }
  if (!theta) { set_error("nlml draw: null output"); return GPT_ERR_BAD_DIMS; }
  return nlml_one_shot(X, N, D, y, Z, b, n, [&](gpt_nlml* h) {
    return gpt_nlml_draw_theta(h, hyper, Lh, S, seed, Zin, theta, nullptr);
  });
}

extern "C" int gpt_gpnt_predict(const double* X, int64_t N, int64_t D, const double* y,
                                const double* Z, const double* b, int64_t n, const double* hyper,
                                int64_t Lh, const double* Xtest, int64_t Ntest, const double* ytest,
                                double* fmu, double* fs2, double* lp) {
  if (!nlml_dims_ok(X, N, D, y, Z, b, n) || !nlml_hyper_ok(hyper, Lh, D) ||
      !test_args_ok("nlml", Xtest, Ntest, ytest, 0, fmu, fs2, lp))
    return GPT_ERR_BAD_DIMS;
  return nlml_one_shot(X, N, D, y, Z, b, n, [&](gpt_nlml* h) {
    return gpt_nlml_predict(h, hyper, Lh, Xtest, Ntest, ytest, 0, fmu, fs2, lp);
  });
}

// ------------------------------------------------------------------ kernel approximation error
// Limits: n <= 8192, N <= 65536 and phi (n × N doubles) at most 2 GiB.
constexpr int64_t kKerrNMax = 8192, kKerrRowsMax = 65536;
constexpr int64_t kKerrPhiBytes = 2LL << 30;

extern "C" int gpt_rff_kernel_error(const double* X, int64_t N, int64_t D, const double* Z,
                                    const double* b, int64_t n, const double* hyper, int64_t Lh,
                                    double* out3) {
  if (!X || !Z || !b || !out3) { set_error("rff_kernel_error: null argument"); return GPT_ERR_BAD_DIMS; }
  if (n < 1 || n > kKerrNMax) { set_error("rff_kernel_error: n must be in 1..8192"); return GPT_ERR_BAD_DIMS; }
  if (N < 1 || N > kKerrRowsMax) { set_error("rff_kernel_error: N must be in 1..65536"); return GPT_ERR_BAD_DIMS; }
  if (D < 1 || D > kDMax) { set_error("rff_kernel_error: D must be in 1..16"); return GPT_ERR_BAD_DIMS; }
  if (8 * n * N > kKerrPhiBytes) {
    set_error("rff_kernel_error: phi (n x N doubles) must not exceed 2 GiB"); return GPT_ERR_BAD_DIMS;
  }
  if (!nlml_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  double lsv[kDMax];
  length_scales(hyper, Lh, (int)D, 2, lsv);
  const double sigma = hyper[Lh - 2];
  const long long nb = (N + kKerrTile - 1) / kKerrTile, ntiles = nb * (nb + 1) / 2;
  DevSet mem;
  double *dX = nullptr, *dZ = nullptr, *db = nullptr, *dls = nullptr, *dphi = nullptr,
         *dpart = nullptr, *dout = nullptr;
  GPT_HIPCHK(mem.upload(&dX, X, (size_t)N * D));
  GPT_HIPCHK(mem.upload(&dZ, Z, (size_t)n * D));
  GPT_HIPCHK(mem.upload(&db, b, (size_t)n));
  GPT_HIPCHK(mem.upload(&dls, (const double*)lsv, (size_t)D));
  GPT_HIPCHK(mem.alloc(&dphi, (size_t)n * N));
  GPT_HIPCHK(mem.alloc(&dpart, 3 * (size_t)ntiles));
  GPT_HIPCHK(mem.alloc(&dout, 4));
  hipStream_t st = nullptr;
  const long long total = (long long)n * N;
  EventTimer tf(&g_rff_ms[0], st);
  hipLaunchKernelGGL(nlml_feature_kernel, dim3((unsigned)std::min((total + 255) / 256, 4096LL)),
                     dim3(256), 0, st, dX, (long long)N, (int)D, dls,
                     std::sqrt(2.0 / (double)n) * sigma, dZ, db, (int)n, dphi, (double*)nullptr);
  tf.stop();
  EventTimer tt(&g_rff_ms[1], st);
  if (n % 2 == 0)
    hipLaunchKernelGGL(kerr_tile_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, st, dphi, dX,
                       dls, (int)n, (int)N, (int)D, sigma * sigma, dpart);
  else
    hipLaunchKernelGGL(kerr_tile_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, st, dphi, dX,
                       dls, (int)n, (int)N, (int)D, sigma * sigma, dpart);
  hipLaunchKernelGGL(kerr_finish_kernel, dim3(1), dim3(64), 0, st, dpart, ntiles, dout);
  tt.stop();
  GPT_HIPCHK(hipGetLastError());
  GPT_HIPCHK(hipMemcpyAsync(out3, dout, 8 * 3, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipStreamSynchronize(st));
  return GPT_OK;
}
