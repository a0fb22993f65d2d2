// Function draws from Gaussian models for MI355X (gfx950): GPrand / GPpost of GaussianProcess.jl
// (:66-122) on the exact GP's factor, and the closed-form RFF posterior over θ.  DESIGN §6h.
//
//   prior      F = L·Z,             L·Lᵀ = K + jitter·I
//   posterior  F = fmu·1ᵀ + L·Z,    L·Lᵀ = Σ + d·I,  Σ = K(X*, X*) − VᵀV,  V = L_A⁻¹·K(X, X*)
//   RFF θ      θ = l·1ᵀ + σ·L⁻ᵀ·Z,  L·Lᵀ = φφᵀ + σ²I   (θ | y ~ N(l, σ²A⁻¹))
//
// Three kernels: the normals Z (Philox stream kGpDraw), the triangular-times-dense product and the
// joint posterior covariance, the last two on v_mfma_f64_16x16x4f64 through mfma_kpair_tile.  The
// factorisations and the solves are exactgp.hip's and nlml.hip's, which also hold the C entries
// (they own the handles).  No atomics; every sum has an order fixed by the shape alone, and an
// output column depends on its own column of Z only, so a draw's bits depend neither on S nor on
// the other columns.
#include "exactgp.h"
#include "host_util.h"
#include "mfma_tile.h"

namespace gpt {

// Z[i + M s] = normal_at(seed, i, s, kGpDraw, kind).  grid (ceil(M/256), S).
__global__ __launch_bounds__(256) void gpd_noise_kernel(double* __restrict__ Z, int M,
                                                        uint64_t seed, uint32_t kind) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t s = blockIdx.y;
  if (i < M) Z[(size_t)i + (size_t)M * s] = normal_at(seed, (uint32_t)i, s, kGpDraw, kind);
}

// A row of the column-major triangular T as an operand of mfma_kpair_tile (its scalar form reads
// p[j] only): entry j of the row from column k0 on, zero outside the triangle's columns lo..hi of
// that row.  What T's storage holds there is never read into a product (the exact GP's factor
// leaves its upper triangle unwritten).
struct GpdTriRow {
  const double* p;
  size_t ld;
  int lo, hi;
  __device__ __forceinline__ double operator[](int j) const {
    return (j >= lo && j <= hi) ? p[ld * (size_t)j] : 0.0;
  }
};

// F[i + M s] = mu_i + c·Σ_k T[i, k]·Z[k + M s].  A wave per 16 × 16 tile of F: row tile
// 4·blockIdx.x + wave, column tile blockIdx.y (columns past S read a clamped column and are not
// stored).  K runs over the tile's part of the triangle in mfma_kpair_tile's blocks of 16: columns
// 0 .. i0 + 15 of a lower T (the tiles right of the diagonal one are skipped, the diagonal one is
// masked per row), i0 .. M − 1 of an upper one.  Lane λ holds F[i0 + (λ>>4) + 4q][s0 + (λ&15)].
template <bool UPPER>
__global__ __launch_bounds__(256) void gpd_trimm_kernel(const double* __restrict__ T, size_t ld,
                                                        int M, const double* __restrict__ Z, int S,
                                                        const double* __restrict__ mu, double c,
                                                        double* __restrict__ F) {
  const int lane = threadIdx.x & 63, li = lane & 15, kl = lane >> 4;
  const int i0 = 16 * (4 * (int)blockIdx.x + uni(threadIdx.x >> 6)), s0 = 16 * (int)blockIdx.y;
  if (i0 >= M) return;
  const int row = min(i0 + li, M - 1), col = min(s0 + li, S - 1);
  const int k0 = UPPER ? i0 : 0, n = M - k0;
  const int kend = UPPER ? n : min(i0 + 16, M);
  const GpdTriRow pa[1] = {{T + (size_t)row + ld * (size_t)k0, ld, UPPER ? row - k0 : 0,
                            UPPER ? n - 1 : row}};
  const double* pb[1] = {Z + (size_t)M * col + k0};
  d4 acc[1][1] = {{d4{0.0, 0.0, 0.0, 0.0}}};
  mfma_kpair_tile<false, 1, 1>(pa, pb, n, kend, kl, acc);
  const int s = s0 + li;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = i0 + kl + 4 * q;
    if (i < M && s < S) F[(size_t)i + (size_t)M * s] = (mu ? mu[i] : 0.0) + c * acc[0][0][q];
  }
}

// Σ[a, b] = k(x*_a, x*_b) − Σ_i V[i, a]·V[i, b] over the lower 64 × 64 blocks: a workgroup per block
// pair, a 32 × 32 tile per wave (egp_syrk_kernel's split), both operands columns of V, contiguous
// in i.  Sig gets Σ + d·I (lower triangle), cov both triangles of Σ.  Lane λ holds
// Σ[a0 + 16t + (λ>>4) + 4q][b0 + 16u + (λ&15)].
template <bool V2>
__global__ __launch_bounds__(256) void gpd_postcov_kernel(const double* __restrict__ V, int N,
                                                          const double* __restrict__ Xt, int Nt,
                                                          EgpHyp H, double d,
                                                          double* __restrict__ Sig,
                                                          double* __restrict__ cov) {
  int bi, bj;
  tri_pair(blockIdx.x, bi, bj);
  const int lane = threadIdx.x & 63, li = lane & 15, kl = lane >> 4;
  const int wv = uni(threadIdx.x >> 6), wi = wv & 1, wj = wv >> 1;
  const int a0 = 64 * bi + 32 * wi, b0 = 64 * bj + 32 * wj;
  if (a0 >= Nt || b0 >= Nt || (bi == bj && wj > wi)) return;
  const double* pa[2];
  const double* pb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    pa[t] = V + (size_t)N * min(a0 + 16 * t + li, Nt - 1);
    pb[t] = V + (size_t)N * min(b0 + 16 * t + li, Nt - 1);
  }
  d4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
  mfma_kpair_tile<V2, 2, 2>(pa, pb, N, N, kl, acc);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int a = a0 + 16 * t + kl + 4 * q, b = b0 + 16 * u + li;
        if (a < Nt && b < Nt && a >= b) {
          const double v = egp_kern(Xt, Nt, a, Xt, Nt, b, H) - acc[t][u][q];
          if (Sig) Sig[(size_t)a + (size_t)Nt * b] = a == b ? v + d : v;
          if (cov) {
            cov[(size_t)a + (size_t)Nt * b] = v;
            cov[(size_t)b + (size_t)Nt * a] = v;
          }
        }
      }
}

hipError_t gpd_normals(double* Z, int M, int S, uint64_t seed, uint32_t kind, const double* Zin,
                       hipStream_t st) {
  if (Zin) return hipMemcpyAsync(Z, Zin, 8 * (size_t)M * S, hipMemcpyHostToDevice, st);
  hipLaunchKernelGGL(gpd_noise_kernel, dim3((M + 255) / 256, S), dim3(256), 0, st, Z, M, seed, kind);
  return hipGetLastError();
}

hipError_t gpd_trimm(const double* T, size_t ld, int M, bool upper, const double* Z, int S,
                     const double* mu, double c, double* F, hipStream_t st) {
  const dim3 grid((M + 63) / 64, (S + 15) / 16);
  if (upper)
    hipLaunchKernelGGL(gpd_trimm_kernel<true>, grid, dim3(256), 0, st, T, ld, M, Z, S, mu, c, F);
  else
    hipLaunchKernelGGL(gpd_trimm_kernel<false>, grid, dim3(256), 0, st, T, ld, M, Z, S, mu, c, F);
  return hipGetLastError();
}

hipError_t gpd_postcov(const double* V, int N, const double* Xt, int Nt, const EgpHyp& H, double d,
                       double* Sig, double* cov, hipStream_t st) {
  const long long nblk = (Nt + 63) / 64;
  const dim3 grid((unsigned)(nblk * (nblk + 1) / 2));
  if (N % 2 == 0)
    hipLaunchKernelGGL(gpd_postcov_kernel<true>, grid, dim3(256), 0, st, V, N, Xt, Nt, H, d, Sig, cov);
  else
    hipLaunchKernelGGL(gpd_postcov_kernel<false>, grid, dim3(256), 0, st, V, N, Xt, Nt, H, d, Sig, cov);
  return hipGetLastError();
}

static thread_local double g_gpd_ms[kGpdPhases] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
double* gpd_phase_ms() { return g_gpd_ms; }

}  // namespace gpt

using namespace gpt;

extern "C" int gpt_gpdraw_last_timing(double* ms, int32_t len) {
  if (!ms || len < 0) { set_error("gpt_gpdraw_last_timing: bad output"); return GPT_ERR_BAD_DIMS; }
  for (int32_t x = 0; x < len; ++x) ms[x] = x < kGpdPhases ? g_gpd_ms[x] : 0.0;
  return GPT_OK;
}
