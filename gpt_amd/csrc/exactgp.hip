// Exact Gaussian-process regression for MI355X (gfx950): squared-exponential kernel (iso or ARD),
// Gaussian noise, zero mean — GP_nlogmarginal (GPT_SGLD.jl:905-915) and GPkit's InfExact /
// prediction, which the reference's experiments use as their quality ceiling.  DESIGN §6d.
//
//   K_ij = σ_RBF² exp(−½ Σ_k ((x_ik − x_jk)/ℓ_k)²),  A = K + σ²I = L·Lᵀ,  z = L⁻¹y,  α = L⁻ᵀz
//   nlml = Σ log L_ii + ½ zᵀz + (N/2) log 2π
//   with W = L⁻¹, P = WᵀW = A⁻¹ and Q = P − ααᵀ:
//     ∂/∂ℓ_k = ½ Σ_ij Q_ij K_ij (x_ik − x_jk)²/ℓ_k³,  ∂/∂σ_RBF = Σ_ij Q_ij K_ij/σ_RBF,  ∂/∂σ² = ½ tr Q
//   fmu = Ksᵀα,  fs2 = max(σ_RBF² − colsum((L⁻¹Ks)²), 0),  lp = −(y − fmu)²/(2 ys2) − ½ log(2π ys2)
//
// Everything is column-major fp64 with leading dimension N.  The factorisation is right-looking in
// panels of kEgpNB = 64 columns, three launches per panel: the diagonal block in one workgroup's
// LDS, the panel rows solved one per thread, and the trailing lower 64 × 64 blocks updated on
// v_mfma_f64_16x16x4f64 by one workgroup each.  The same 32 × 32 MFMA tile (egp_gemm_tile) updates
// the rows below a solved block of the many-right-hand-side triangular solve, which serves the
// prediction (B = Ks) and L⁻¹ (B = I, only the columns left of the panel's end).  No atomics;
// every sum has an order fixed by the shape alone, and every loop a trip count fixed by N, so a
// failed factorisation runs to the end with NaNs and a status word.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "device_util.h"
#include "exactgp.h"
#include "host_util.h"

namespace gpt {

constexpr int kEgpNMax = 16384;     // three N × N fp64 buffers: 6.4 GB
constexpr int kEgpNB = 64;          // panel width (chosen from 16, 32, 64, 128)
constexpr int kEgpLs = kEgpNB + 1;  // LDS row stride of a diagonal block
constexpr int kEgpPart = kDMax + 2; // per-workgroup partial sums of the gradient pass
constexpr int kEgpChunk = 1024;     // test columns per prediction chunk when the caller passes 0
constexpr int kEgpChunkMax = 4096;
static_assert(64 % kNW == 0, "egp_grad_kernel splits 64 columns over the waves");

// 1. A (lower 64 × 64 blocks) = K + σ²I from X.  grid (nblk, nblk); blocks above the diagonal leave.
__global__ __launch_bounds__(256) void egp_build_kernel(const double* __restrict__ X, int N,
                                                        EgpHyp H, double* __restrict__ A) {
  if (blockIdx.y > blockIdx.x) return;
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  if (i >= N) return;
  for (int jj = threadIdx.x >> 6; jj < 64; jj += 4) {
    const int j = blockIdx.y * 64 + jj;
    if (j < N && j <= i)
      A[(size_t)i + (size_t)N * j] = egp_kern(X, N, i, X, N, j, H) + (i == j ? H.s2 : 0.0);
  }
}

// Ks[i + N c] = k(x_i, xtest_{c0 + c}) for c < nc.  grid (ceil(N/64), ceil(nc/16)).
__global__ __launch_bounds__(256) void egp_cross_kernel(const double* __restrict__ X, int N,
                                                        const double* __restrict__ Xt,
                                                        long long Ntest, long long c0, int nc,
                                                        EgpHyp H, double* __restrict__ Ks) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  if (i >= N) return;
  for (int u = 0; u < 4; ++u) {
    const int c = blockIdx.y * 16 + (threadIdx.x >> 6) + 4 * u;
    if (c < nc) Ks[(size_t)i + (size_t)N * c] = egp_kern(X, N, i, Xt, Ntest, c0 + c, H);
  }
}

// 2a. The diagonal block A[j0.., j0..] (nb <= 64 rows) factored in LDS by one workgroup: per
// column the pivot's square root, the column scaled by its reciprocal (dpotf2's form), then the
// rank-1 update of the lower triangle to its right, an element per thread and pass.  (Rows in one
// wave's registers, chol_blk_kernel's scheme, do not carry over to 64 columns: 2016 unrolled
// multiplier broadcasts spill either the scalars or the row.)  A block narrower than 64 is padded
// with the identity.  status = 1 at a pivot that is not positive; the loops do not depend on it.
__global__ __launch_bounds__(256) void egp_potf2_kernel(double* __restrict__ A, int N, int j0,
                                                        int32_t* __restrict__ status) {
  __shared__ double S[kEgpNB * kEgpLs];
  __shared__ int badflag;
  const int tid = threadIdx.x, nb = min(kEgpNB, N - j0);
  if (tid == 0) badflag = 0;
  for (int e = tid; e < kEgpNB * kEgpNB; e += 256) {
    const int r = e & 63, c = e >> 6;
    const double v = A[(size_t)(j0 + min(r, nb - 1)) + (size_t)N * (j0 + min(c, nb - 1))];
    S[r * kEgpLs + c] = (r < nb && c < nb) ? (c <= r ? v : 0.0) : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int j = 0; j < kEgpNB; ++j) {
    const double d = S[j * kEgpLs + j];
    const double pv = sqrt(d), rp = 1.0 / pv;
    __syncthreads();                                   // every thread has read the pivot
    if (tid == 0 && !(d > 0.0)) badflag = 1;
    if (tid >= j && tid < kEgpNB) S[tid * kEgpLs + j] = tid == j ? pv : S[tid * kEgpLs + j] * rp;
    __syncthreads();
    const int w = kEgpNB - 1 - j;                      // columns j+1 .. 63, rows k .. 63 of each
    for (int e = tid; e < w * kEgpNB; e += 256) {
      const int i = e & 63, k = j + 1 + (e >> 6);
      if (i >= k) S[i * kEgpLs + k] -= S[i * kEgpLs + j] * S[k * kEgpLs + j];
    }
    __syncthreads();
  }
  if (tid == 0 && badflag) *status = 1;
  for (int e = tid; e < kEgpNB * kEgpNB; e += 256) {
    const int r = e & 63, c = e >> 6;
    if (r < nb && c <= r) A[(size_t)(j0 + r) + (size_t)N * (j0 + c)] = S[r * kEgpLs + c];
  }
}

// The nb × nb lower triangle at (j0, j0) of L into LDS (row stride kEgpLs), padded with the
// identity to 64 × 64, and the reciprocals of its diagonal.  Called by every thread of the block.
__device__ __forceinline__ void egp_load_tri(const double* __restrict__ L, int N, int j0, int nb,
                                             double* Ls, double* rinv) {
  for (int e = threadIdx.x; e < kEgpNB * kEgpNB; e += blockDim.x) {
    const int r = e & 63, c = e >> 6;
    const double v = L[(size_t)(j0 + min(r, nb - 1)) + (size_t)N * (j0 + min(c, nb - 1))];
    Ls[r * kEgpLs + c] = (r < nb && c < nb) ? (c <= r ? v : 0.0) : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int r = threadIdx.x; r < kEgpNB; r += blockDim.x) rinv[r] = 1.0 / Ls[r * kEgpLs + r];
  __syncthreads();
}

// x := T⁻¹x for the 64 × 64 lower triangle in LDS: every T read is a broadcast.
__device__ __forceinline__ void egp_fwd64(double (&x)[kEgpNB], const double* Ls,
                                          const double* rinv) {
#pragma unroll
  for (int j = 0; j < kEgpNB; ++j) {
    double s = x[j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= x[k] * Ls[j * kEgpLs + k];
    x[j] = s * rinv[j];
  }
}

// 2b. L21 = A21·L11⁻ᵀ: a thread per row below a full panel (row i of L21 solves L11·x = a_iᵀ).
__global__ __launch_bounds__(256) void egp_panel_kernel(double* __restrict__ A, int N, int j0) {
  __shared__ double Ls[kEgpNB * kEgpLs];
  __shared__ double rinv[kEgpNB];
  egp_load_tri(A, N, j0, kEgpNB, Ls, rinv);
  const int i = j0 + kEgpNB + blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double* row = A + (size_t)i + (size_t)N * j0;
  double x[kEgpNB];
#pragma unroll
  for (int k = 0; k < kEgpNB; ++k) x[k] = row[(size_t)N * k];
  egp_fwd64(x, Ls, rinv);
#pragma unroll
  for (int k = 0; k < kEgpNB; ++k) row[(size_t)N * k] = x[k];
}

// The GEMM tile of the trailing update and of the triangular solve: one wave,
//   C[i, c] −= Σ_{k < 64} pa[i + lda·k] · pb[c·sbc + k·sbk],  i in [i0, i0 + 32), c in [c0, c0 + 32),
// on v_mfma_f64_16x16x4f64, 2 × 2 tiles, K in 16 steps.  The column operand goes first, so lane λ
// holds C[i0 + 16t + (λ&15)][c0 + 16u + (λ>>4) + 4q]: every access of C covers 16 consecutive rows.
// Rows >= ilim and columns >= clim read a clamped address and are not stored (a row of C depends
// on its own operand row alone); `lower` stores i >= c only.
__device__ __forceinline__ void egp_gemm_tile(const double* __restrict__ pa, size_t lda,
                                              const double* __restrict__ pb, size_t sbc, size_t sbk,
                                              double* __restrict__ C, size_t ldc, int i0, int ilim,
                                              int c0, int clim, bool lower) {
  const int lane = threadIdx.x & 63, li = lane & 15, kl = lane >> 4;
  const double* ar[2];
  const double* bc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    ar[t] = pa + (size_t)min(i0 + 16 * t + li, ilim - 1) + lda * kl;
    bc[t] = pb + (size_t)min(c0 + 16 * t + li, clim - 1) * sbc + sbk * kl;
  }
  d4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int s = 0; s < kEgpNB / 4; ++s) {
    double a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[t] = ar[t][lda * 4 * s];
      b[t] = bc[t][sbk * 4 * s];
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[u], a[t], acc[t][u], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + 16 * t + li, c = c0 + 16 * u + kl + 4 * q;
        if (i < ilim && c < clim && (!lower || i >= c)) {
          double* p = C + (size_t)i + ldc * c;
          *p = *p - acc[t][u][q];
        }
      }
}

// 2c. A22 −= L21·L21ᵀ over the lower 64 × 64 blocks behind a full panel: a workgroup per block
// pair, a 32 × 32 tile per wave.
__global__ __launch_bounds__(256) void egp_syrk_kernel(double* __restrict__ A, int N, int j0) {
  int bi, bj;
  tri_pair(blockIdx.x, bi, bj);
  const int wv = uni(threadIdx.x >> 6), wi = wv & 1, wj = wv >> 1;
  const int r0 = j0 + kEgpNB, i0 = r0 + 64 * bi + 32 * wi, c0 = r0 + 64 * bj + 32 * wj;
  if (i0 >= N || c0 >= N || (bi == bj && wj > wi)) return;
  const double* pan = A + (size_t)N * j0;
  egp_gemm_tile(pan, N, pan, 1, N, A, N, i0, N, c0, N, true);
}

// 3a. Rows j0 .. j0 + nb − 1 of B := L11⁻¹ · (those rows) for 64 columns c < ncols per workgroup
// (one wave).  The block of B goes through LDS (coalesced over the rows on both sides, row stride
// 65); a thread then holds its column in registers and solves it against the packed triangle
// (T[j(j+1)/2 + k], every read a broadcast at a compile-time offset; the diagonal holds
// reciprocals).  A block narrower than 64 is padded with the identity.  ident: B stands for the
// identity where it has not been written yet (columns c >= j0 of L⁻¹).  The launch bound is 256
// for its register budget (512 let the scheduler hoist the triangle's reads and spill them).
__global__ __launch_bounds__(256) void egp_trsm_diag_kernel(const double* __restrict__ L, int N,
                                                            int j0, double* __restrict__ B,
                                                            size_t ldb, int ncols, int ident) {
  __shared__ double Tp[kEgpNB * (kEgpNB + 1) / 2];
  __shared__ double Bt[kEgpNB * kEgpLs];
  const int nb = min(kEgpNB, N - j0), tid = threadIdx.x, cbase = blockIdx.x * 64;
  for (int e = tid; e < kEgpNB * kEgpNB; e += 64) {
    const int r = e & 63, c = e >> 6;
    if (c <= r) {
      const double v = L[(size_t)(j0 + min(r, nb - 1)) + (size_t)N * (j0 + min(c, nb - 1))];
      const double t = (r < nb && c < nb) ? v : (r == c ? 1.0 : 0.0);
      Tp[r * (r + 1) / 2 + c] = r == c ? 1.0 / t : t;
    }
  }
  for (int e = tid; e < kEgpNB * kEgpNB; e += 64) {
    const int k = e & 63, cc = e >> 6, c = cbase + cc;
    double v = 0.0;
    if (c < ncols && k < nb) {
      if (ident && c >= j0) v = (k == c - j0) ? 1.0 : 0.0;
      else v = B[(size_t)(j0 + k) + ldb * c];
    }
    Bt[k * kEgpLs + cc] = v;
  }
  __syncthreads();
  {
    double x[kEgpNB];
#pragma unroll
    for (int k = 0; k < kEgpNB; ++k) x[k] = Bt[k * kEgpLs + tid];
#pragma unroll
    for (int j = 0; j < kEgpNB; ++j) {
      double s = x[j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= x[k] * Tp[j * (j + 1) / 2 + k];
      x[j] = s * Tp[j * (j + 1) / 2 + j];
    }
#pragma unroll
    for (int k = 0; k < kEgpNB; ++k) Bt[k * kEgpLs + tid] = x[k];
  }
  __syncthreads();
  for (int e = tid; e < kEgpNB * kEgpNB; e += 64) {
    const int k = e & 63, cc = e >> 6, c = cbase + cc;
    if (c < ncols && k < nb) B[(size_t)(j0 + k) + ldb * c] = Bt[k * kEgpLs + cc];
  }
}

// 3b. The rows of B below a full solved block: B[i, c] −= Σ_k L[i, j0 + k]·B[j0 + k, c].
// grid (ceil((N − j0 − 64)/64), ceil(ncols/64)).
__global__ __launch_bounds__(256) void egp_trsm_upd_kernel(const double* __restrict__ L, int N,
                                                           int j0, double* __restrict__ B,
                                                           size_t ldb, int ncols) {
  const int wv = uni(threadIdx.x >> 6), wi = wv & 1, wj = wv >> 1;
  const int i0 = j0 + kEgpNB + 64 * blockIdx.x + 32 * wi, c0 = 64 * blockIdx.y + 32 * wj;
  if (i0 >= N || c0 >= ncols) return;
  egp_gemm_tile(L + (size_t)N * j0, N, B + j0, ldb, 1, B, ldb, i0, N, c0, ncols, false);
}

// Vector solves for z = L⁻¹y and α = L⁻ᵀz, one launch per block of 64 unknowns: wave 0 of every
// workgroup solves the block's triangle in registers (trsv_blk_kernel's scheme; the workgroups
// repeat it rather than wait for one another), workgroup 0 writes the block of the solution to
// `out`, and every thread takes the block out of one remaining entry of the right-hand side r
// (forward: the rows below, transposed: the rows above).  r's entries of the block itself are only
// read in this launch.
template <int TRANS>
__global__ __launch_bounds__(256) void egp_trsv_kernel(const double* __restrict__ L, int N, int j0,
                                                       double* __restrict__ r,
                                                       double* __restrict__ out) {
  __shared__ double xs[kEgpNB];
  const int tid = threadIdx.x, lane = tid & 63, nb = min(kEgpNB, N - j0);
  if (uni(tid >> 6) == 0) {
    const bool rok = lane < nb;
    const int lr = j0 + min(lane, nb - 1);
    double rw[kEgpNB];
#pragma unroll
    for (int k = 0; k < kEgpNB; ++k) {
      const int kc = j0 + min(k, nb - 1);
      const double v = TRANS ? L[(size_t)kc + (size_t)N * lr] : L[(size_t)lr + (size_t)N * kc];
      const bool tri = TRANS ? k >= lane : k <= lane;
      rw[k] = (rok && k < nb) ? (tri ? v : 0.0) : (k == lane ? 1.0 : 0.0);
    }
    double xv = rok ? r[lr] : 0.0;
    if (!TRANS) {
#pragma unroll
      for (int j = 0; j < kEgpNB; ++j) {
        const double xj = readlane_d(xv, j) / readlane_d(rw[j], j);
        if (lane == j) xv = xj;
        if (lane > j) xv -= rw[j] * xj;
      }
    } else {
#pragma unroll
      for (int j = kEgpNB - 1; j >= 0; --j) {
        const double xj = readlane_d(xv, j) / readlane_d(rw[j], j);
        if (lane == j) xv = xj;
        if (lane < j) xv -= rw[j] * xj;
      }
    }
    xs[lane] = xv;
    if (blockIdx.x == 0 && rok) out[j0 + lane] = xv;
  }
  __syncthreads();
  if (!TRANS) {
    const int i = j0 + nb + blockIdx.x * 256 + tid;
    if (i < N) {
      double s = r[i];
      for (int k = 0; k < nb; ++k) s -= L[(size_t)i + (size_t)N * (j0 + k)] * xs[k];
      r[i] = s;
    }
  } else {
    const int i = blockIdx.x * 256 + tid;
    if (i < j0) {
      double s = r[i];
      const double* lc = L + (size_t)j0 + (size_t)N * i;
      for (int k = nb - 1; k >= 0; --k) s -= lc[k] * xs[k];
      r[i] = s;
    }
  }
}

// out = {Σ log L_ii, zᵀz}
__global__ __launch_bounds__(kNT) void egp_scalars_kernel(const double* __restrict__ L,
                                                          const double* __restrict__ z, int N,
                                                          double* __restrict__ out) {
  __shared__ double red[kNW];
  double ld = 0.0, zz = 0.0;
  for (int i = threadIdx.x; i < N; i += kNT) {
    ld += log(L[(size_t)i + (size_t)N * i]);
    zz = fma(z[i], z[i], zz);
  }
  const double a = blk_sum(ld, red), b = blk_sum(zz, red);
  if (threadIdx.x == 0) { out[0] = a; out[1] = b; }
}

// 4a. P = WᵀW (lower 32 × 32 blocks, both triangles of the diagonal ones) for the lower-triangular
// W = L⁻¹ whose upper part is zero: P[a, b] = Σ_{i >= a0} W[i, a]·W[i, b], a0 the block's first
// row.  A wave per block pair; both operands are contiguous in i, a lane takes the rows
// i + 2(λ>>4) + {0, 1} of each step of 8 for two MFMAs.  Lane λ holds P[a0 + 16t + (λ&15)]
// [b0 + 16u + (λ>>4) + 4q].  Rows past N are selected to zero in one operand.
__global__ __launch_bounds__(256) void egp_ptp_kernel(const double* __restrict__ W, int N,
                                                      double* __restrict__ P) {
  const int lane = threadIdx.x & 63, li = lane & 15, kl = lane >> 4;
  const int T = (N + 31) / 32;
  const long long task = (long long)blockIdx.x * 4 + uni(threadIdx.x >> 6);
  if (task >= (long long)T * (T + 1) / 2) return;
  int ba, bb;
  tri_pair(task, ba, bb);
  const int a0 = 32 * ba, b0 = 32 * bb;
  const double* wa[2];
  const double* wb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    wa[t] = W + (size_t)N * min(a0 + 16 * t + li, N - 1);
    wb[t] = W + (size_t)N * min(b0 + 16 * t + li, N - 1);
  }
  d4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
  for (int ib = a0; ib < N; ib += 8) {
    const int i1 = ib + 2 * kl, i2 = i1 + 1;
    const int c1 = min(i1, N - 1), c2 = min(i2, N - 1);
    double a1[2], a2[2], b1[2], b2[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a1[t] = i1 < N ? wa[t][c1] : 0.0;
      a2[t] = i2 < N ? wa[t][c2] : 0.0;
      b1[t] = wb[t][c1];
      b2[t] = wb[t][c2];
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1[u], a1[t], acc[t][u], 0, 0, 0);
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(b2[u], a2[t], acc[t][u], 0, 0, 0);
      }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int a = a0 + 16 * t + li, b = b0 + 16 * u + kl + 4 * q;
        if (a < N && b < N) P[(size_t)a + (size_t)N * b] = acc[t][u][q];
      }
}

// 4b. The gradient pass over the lower 64 × 64 blocks: K_ij again from X, Q_ij = P_ij − α_i α_j,
// weight 2 below the diagonal and 1 on it.  A thread holds row i and walks 64/kNW columns; the
// workgroup's sums (blk_sum's fixed pattern) go to part[block][0] = Σ Q K, [1 + k] = Σ Q K
// (x_ik − x_jk)², [kDMax + 1] = Σ_i Q_ii.  Entries above the diagonal are never read into a sum
// (P has none there).
template <int DP>
__global__ __launch_bounds__(kNT) void egp_grad_kernel(const double* __restrict__ P,
                                                       const double* __restrict__ alpha,
                                                       const double* __restrict__ X, int N,
                                                       EgpHyp H, double* __restrict__ part) {
  __shared__ double xj[64 * DP];
  __shared__ double aj[64];
  __shared__ double red[kNW];
  int bi, bj;
  tri_pair(blockIdx.x, bi, bj);
  const int tid = threadIdx.x, i = 64 * bi + (tid & 63), j0 = 64 * bj;
  for (int e = tid; e < 64 * DP; e += kNT) {
    const int jj = e & 63, k = e >> 6, j = j0 + jj;
    xj[jj * DP + k] = (j < N && k < H.D) ? X[(size_t)j + (size_t)N * k] : 0.0;
  }
  for (int jj = tid; jj < 64; jj += kNT) aj[jj] = j0 + jj < N ? alpha[j0 + jj] : 0.0;
  __syncthreads();
  const bool iok = i < N;
  const int ic = iok ? i : N - 1;
  double xi[DP], il[DP], acc[DP + 2];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    xi[k] = k < H.D ? X[(size_t)ic + (size_t)N * k] : 0.0;
    il[k] = k < H.D ? H.invl[k] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < DP + 2; ++q) acc[q] = 0.0;
  const double ai = alpha[ic];
  constexpr int CW = 64 / kNW;
  for (int u = 0; u < CW; ++u) {
    const int jj = (tid >> 6) * CW + u, j = j0 + jj;
    const bool ok = iok && j < N && j <= i;
    const double p = P[(size_t)ic + (size_t)N * min(j, N - 1)];
    double dd[DP], s = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const double d = xi[k] - xj[jj * DP + k];
      dd[k] = d * d;
      const double dl = d * il[k];
      s = fma(dl, dl, s);
    }
    const double q = p - ai * aj[jj];
    const double qk = ok ? (i == j ? 1.0 : 2.0) * q * (H.sig2 * exp(-0.5 * s)) : 0.0;
    acc[0] += qk;
#pragma unroll
    for (int k = 0; k < DP; ++k) acc[1 + k] = fma(qk, dd[k], acc[1 + k]);
    acc[DP + 1] += (ok && i == j) ? q : 0.0;
  }
  double* out = part + (size_t)blockIdx.x * kEgpPart;
#pragma unroll
  for (int q = 0; q < DP + 2; ++q) {
    const double v = blk_sum(acc[q], red);
    if (tid == 0) out[q == DP + 1 ? kDMax + 1 : q] = v;
  }
}

// out[q] = Σ_blocks part[block][q] for q = 0 .. D and kDMax + 1: the blocks strided over the
// threads in block order, then blk_sum (nlml_finish_kernel's pattern).
__global__ __launch_bounds__(kNT) void egp_finish_kernel(const double* __restrict__ part,
                                                         long long nblk, int D,
                                                         double* __restrict__ out) {
  __shared__ double red[kNW];
  for (int q = 0; q < D + 2; ++q) {
    const int slot = q == D + 1 ? kDMax + 1 : q;
    double s = 0.0;
    for (long long b = threadIdx.x; b < nblk; b += kNT) s += part[(size_t)b * kEgpPart + slot];
    const double tot = blk_sum(s, red);
    if (threadIdx.x == 0) out[slot] = tot;
  }
}

// 5. Prediction epilogue, a wave per test column c of the chunk (lanes over the training rows,
// wave_sum's fixed pattern: a column's result does not depend on the chunk it came in).
// mode 0: fmu[c] = Σ_i Ks[i, c] α_i (before the solve overwrites Ks); mode 1: fs2[c] =
// max(σ_RBF² − Σ_i V[i, c]², 0) and, with targets, lp[c].
__global__ __launch_bounds__(256) void egp_pred_kernel(const double* __restrict__ M, int N, int nc,
                                                       const double* __restrict__ alpha, int mode,
                                                       double sig2, double s2,
                                                       const double* __restrict__ ytest,
                                                       double* __restrict__ fmu,
                                                       double* __restrict__ fs2,
                                                       double* __restrict__ lp) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + uni(threadIdx.x >> 6);
  if (c >= nc) return;
  const double* col = M + (size_t)N * c;
  double s = 0.0;
  if (mode == 0) {
    for (int i = lane; i < N; i += 64) s = fma(col[i], alpha[i], s);
  } else {
    for (int i = lane; i < N; i += 64) s = fma(col[i], col[i], s);
  }
  s = wave_sum(s);
  if (lane != 0) return;
  if (mode == 0) {
    fmu[c] = s;
  } else {
    const double v = fmax(sig2 - s, 0.0);
    fs2[c] = v;
    if (lp) {
      const double ys2 = v + s2, d = ytest[c] - fmu[c];
      lp[c] = -(d * d) / (2.0 * ys2) - 0.5 * log(2.0 * M_PI * ys2);
    }
  }
}

}  // namespace gpt

using namespace gpt;

// ------------------------------------------------------------------------------ host side
#include "gp_handle.h"

constexpr int kEgpPhases = 6;        // build, Cholesky, solves, inverse, P, gradient pass
struct gpt_egp {
  int N = 0, D = 0;
  double *X = nullptr, *y = nullptr, *A = nullptr, *W = nullptr, *P = nullptr, *r = nullptr,
         *z = nullptr, *alpha = nullptr, *part = nullptr, *sums = nullptr, *scal = nullptr;
  int32_t* status = nullptr;
  FactorKey factor;                    // A holds L and alpha the weights of these hyper-parameters
  DevSet mem;
  GrowBlock Ks;                        // regrown when a call asks for more columns
  PhaseMarks marks;                    // gpt_egp_eval_timed's
};

static bool egp_dims_ok(const void* X, int64_t N, int64_t D, const void* y) {
  if (!X || !y) { set_error("exact GP: null input array"); return false; }
  if (N < 1 || N > kEgpNMax) { set_error("exact GP: N must be in 1..16384"); return false; }
  if (D < 1 || D > kDMax) { set_error("exact GP: D must be in 1..16"); return false; }
  return true;
}

static bool egp_hyper_ok(const double* hyper, int64_t Lh, int64_t D) {
  return hyper_ok("exact GP", hyper, Lh, D, 2);
}

extern "C" int gpt_egp_create(const double* X, int64_t N, int64_t D, const double* y,
                              gpt_egp** out) {
  if (!out) { set_error("exact GP: null handle pointer"); return GPT_ERR_BAD_DIMS; }
  *out = nullptr;
  if (!egp_dims_ok(X, N, D, y)) return GPT_ERR_BAD_DIMS;
  std::unique_ptr<gpt_egp> h(new gpt_egp);
  h->N = (int)N; h->D = (int)D;
  const size_t nblk = (size_t)((N + 63) / 64);
  DevSet& M = h->mem;
  GPT_HIPCHK(M.upload(&h->X, X, (size_t)N * D));
  GPT_HIPCHK(M.upload(&h->y, y, (size_t)N));
  GPT_HIPCHK(M.alloc(&h->A, (size_t)N * N));
  GPT_HIPCHK(M.alloc(&h->r, (size_t)N));
  GPT_HIPCHK(M.alloc(&h->z, (size_t)N));
  GPT_HIPCHK(M.alloc(&h->alpha, (size_t)N));
  GPT_HIPCHK(M.alloc(&h->part, nblk * (nblk + 1) / 2 * kEgpPart));
  GPT_HIPCHK(M.alloc(&h->sums, (size_t)kEgpPart));
  GPT_HIPCHK(M.alloc(&h->scal, 2));
  GPT_HIPCHK(M.alloc(&h->status, 4));
  *out = h.release();
  return GPT_OK;
}

extern "C" int gpt_egp_destroy(gpt_egp* h) { return destroy_handle(h); }

// The one-shot forms: create, body on the fresh handle, destroy.
template <class Body>
static int egp_one_shot(const double* X, int64_t N, int64_t D, const double* y, Body&& body) {
  return one_shot<gpt_egp>([&](gpt_egp** h) { return gpt_egp_create(X, N, D, y, h); }, body);
}

static EgpHyp egp_hyp(const double* hyper, int64_t Lh, int D) {
  EgpHyp H;
  double ls[kDMax];
  length_scales(hyper, Lh, D, 2, ls);
  for (int k = 0; k < kDMax; ++k) H.invl[k] = k < D ? 1.0 / ls[k] : 0.0;
  H.sig2 = hyper[Lh - 2] * hyper[Lh - 2];
  H.s2 = hyper[Lh - 1];
  H.D = D;
  return H;
}

// X := L⁻¹B for the ncols columns of B (leading dimension N): per block of 64 rows, the block's
// solve and the update of the rows below.  ident: B = I, column c enters at its own block.
static hipError_t egp_trsm(const double* L, int N, double* B, int ncols, bool ident,
                           hipStream_t st) {
  for (int j0 = 0; j0 < N; j0 += kEgpNB) {
    const int nc = ident ? std::min(N, j0 + kEgpNB) : ncols;
    hipLaunchKernelGGL(egp_trsm_diag_kernel, dim3((nc + 63) / 64), dim3(64), 0, st, L, N, j0, B,
                       (size_t)N, nc, ident ? 1 : 0);
    const int rem = N - j0 - kEgpNB;
    if (rem > 0)
      hipLaunchKernelGGL(egp_trsm_upd_kernel, dim3((rem + 63) / 64, (nc + 63) / 64), dim3(256), 0,
                         st, L, N, j0, B, (size_t)N, nc);
  }
  return hipGetLastError();
}

// A (N × N, lower 64 × 64 blocks, leading dimension N) := its Cholesky factor, panel by panel:
// the diagonal block, the rows below it, the trailing update.  *status = 1 at a pivot that is not
// positive.  The factorisation of every matrix here: K + σ²I, and the draws' K + jitter·I and Σ.
static hipError_t egp_chol(double* A, int N, int32_t* status, hipStream_t st) {
  for (int j0 = 0; j0 < N; j0 += kEgpNB) {
    hipLaunchKernelGGL(egp_potf2_kernel, dim3(1), dim3(256), 0, st, A, N, j0, status);
    const int rem = N - j0 - kEgpNB;
    if (rem > 0) {
      hipLaunchKernelGGL(egp_panel_kernel, dim3((rem + 255) / 256), dim3(256), 0, st, A, N, j0);
      const long long T = (rem + 63) / 64;
      hipLaunchKernelGGL(egp_syrk_kernel, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, st, A,
                         N, j0);
    }
  }
  return hipGetLastError();
}

static int egp_eval_impl(gpt_egp* h, const double* hyper, int64_t Lh, int32_t want_grad,
                         double* nlml, double* grad, double* alpha_out, double* phase_ms) {
  if (!h || !nlml || (want_grad && !grad)) {
    set_error("exact GP: null handle or output"); return GPT_ERR_BAD_DIMS;
  }
  if (!egp_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  const int N = h->N, D = h->D;
  const EgpHyp H = egp_hyp(hyper, Lh, D);
  hipStream_t st = nullptr;
  h->factor.clear();
  if (want_grad && !h->W) {
    GPT_HIPCHK(h->mem.alloc(&h->W, (size_t)N * N));
    GPT_HIPCHK(h->mem.alloc(&h->P, (size_t)N * N));
  }
  GPT_HIPCHK(h->marks.begin(phase_ms != nullptr, kEgpPhases));
  auto mark = [&]() { h->marks.mark(st); };
  const int nblk = (N + 63) / 64;
  const long long npair = (long long)nblk * (nblk + 1) / 2;
  GPT_HIPCHK(hipMemsetAsync(h->status, 0, 16, st));
  mark();
  hipLaunchKernelGGL(egp_build_kernel, dim3(nblk, nblk), dim3(256), 0, st, h->X, N, H, h->A);
  GPT_HIPCHK(hipGetLastError());
  mark();
  GPT_HIPCHK(egp_chol(h->A, N, h->status, st));
  mark();
  GPT_HIPCHK(hipMemcpyAsync(h->r, h->y, 8 * (size_t)N, hipMemcpyDeviceToDevice, st));
  for (int j0 = 0; j0 < N; j0 += kEgpNB) {
    const int rem = std::max(N - j0 - kEgpNB, 1);
    hipLaunchKernelGGL(egp_trsv_kernel<0>, dim3((rem + 255) / 256), dim3(256), 0, st, h->A, N, j0,
                       h->r, h->z);
  }
  GPT_HIPCHK(hipMemcpyAsync(h->r, h->z, 8 * (size_t)N, hipMemcpyDeviceToDevice, st));
  for (int j0 = (N - 1) / kEgpNB * kEgpNB; j0 >= 0; j0 -= kEgpNB)
    hipLaunchKernelGGL(egp_trsv_kernel<1>, dim3((std::max(j0, 1) + 255) / 256), dim3(256), 0, st,
                       h->A, N, j0, h->r, h->alpha);
  hipLaunchKernelGGL(egp_scalars_kernel, dim3(1), dim3(kNT), 0, st, h->A, h->z, N, h->scal);
  GPT_HIPCHK(hipGetLastError());
  mark();
  if (want_grad) {
    GPT_HIPCHK(hipMemsetAsync(h->W, 0, 8 * (size_t)N * N, st));
    GPT_HIPCHK(egp_trsm(h->A, N, h->W, N, true, st));
    mark();
    const long long T = (N + 31) / 32;
    hipLaunchKernelGGL(egp_ptp_kernel, dim3((unsigned)((T * (T + 1) / 2 + 3) / 4)), dim3(256), 0,
                       st, h->W, N, h->P);
    GPT_HIPCHK(hipGetLastError());
    mark();
#define EGP_GRAD(DP)                                                                            \
  hipLaunchKernelGGL((egp_grad_kernel<DP>), dim3((unsigned)npair), dim3(kNT), 0, st, h->P, \
                     h->alpha, h->X, N, H, h->part)
    if (D <= 1) EGP_GRAD(1);
    else if (D <= 2) EGP_GRAD(2);
    else if (D <= 4) EGP_GRAD(4);
    else if (D <= 8) EGP_GRAD(8);
    else EGP_GRAD(16);
#undef EGP_GRAD
    hipLaunchKernelGGL(egp_finish_kernel, dim3(1), dim3(kNT), 0, st, h->part, npair, D, h->sums);
    GPT_HIPCHK(hipGetLastError());
    mark();
  } else {
    for (int q = 0; q < 3; ++q) mark();
  }
  double sc[2], sums[kEgpPart];
  int32_t bad = 0;
  std::vector<double> ah(alpha_out ? N : 0);
  GPT_HIPCHK(hipMemcpyAsync(sc, h->scal, 8 * 2, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipMemcpyAsync(&bad, h->status, 4, hipMemcpyDeviceToHost, st));
  if (alpha_out) GPT_HIPCHK(hipMemcpyAsync(ah.data(), h->alpha, 8 * (size_t)N, hipMemcpyDeviceToHost, st));
  if (want_grad) GPT_HIPCHK(hipMemcpyAsync(sums, h->sums, 8 * kEgpPart, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipStreamSynchronize(st));
  GPT_HIPCHK(h->marks.read(phase_ms));
  if (bad) {
    nan_fill(nlml, 1);
    if (want_grad) nan_fill(grad, Lh);
    nan_fill(alpha_out, N);
    set_error("exact GP: K + signal_var*I is not positive definite (PosDefException)");
    return GPT_ERR_NOT_SPD;
  }
  *nlml = sc[0] + 0.5 * sc[1] + 0.5 * (double)N * std::log(2 * M_PI);
  if (want_grad) {
    const double sigma = hyper[Lh - 2];
    double ls[kDMax], gl[kDMax];
    length_scales(hyper, Lh, D, 2, ls);
    for (int k = 0; k < D; ++k) gl[k] = 0.5 * sums[1 + k] / (ls[k] * ls[k] * ls[k]);
    fold_ls_grad(gl, D, Lh, 2, grad);
    grad[Lh - 2] = sums[0] / sigma;
    grad[Lh - 1] = 0.5 * sums[kDMax + 1];
  }
  if (alpha_out) std::memcpy(alpha_out, ah.data(), 8 * (size_t)N);
  h->factor.set(hyper, Lh);
  return GPT_OK;
}

// The factor of hyper in A and its weights in alpha: the resident ones when they are those of
// these bits, else an evaluation without gradient.
static int egp_ensure_factor(gpt_egp* h, const double* hyper, int64_t Lh) {
  if (h->factor.matches(hyper, Lh)) return GPT_OK;
  double val = 0.0;
  return egp_eval_impl(h, hyper, Lh, 0, &val, nullptr, nullptr, nullptr);
}

extern "C" int gpt_egp_eval(gpt_egp* h, const double* hyper, int64_t Lh, int32_t want_grad,
                            double* nlml, double* grad, double* alpha) {
  return egp_eval_impl(h, hyper, Lh, want_grad, nlml, grad, alpha, nullptr);
}

extern "C" int gpt_egp_eval_timed(gpt_egp* h, const double* hyper, int64_t Lh, int32_t want_grad,
                                  double* nlml, double* grad, double* phase_ms) {
  if (!phase_ms) { set_error("exact GP: null phase_ms"); return GPT_ERR_BAD_DIMS; }
  return egp_eval_impl(h, hyper, Lh, want_grad, nlml, grad, nullptr, phase_ms);
}

extern "C" int gpt_egp_predict(gpt_egp* h, const double* hyper, int64_t Lh, const double* Xtest,
                               int64_t Ntest, const double* ytest, int64_t chunk, double* fmu,
                               double* fs2, double* lp) {
  if (!h) { set_error("exact GP: null handle"); return GPT_ERR_BAD_DIMS; }
  if (!egp_hyper_ok(hyper, Lh, h->D) ||
      !test_args_ok("exact GP", Xtest, Ntest, ytest, chunk, fmu, fs2, lp))
    return GPT_ERR_BAD_DIMS;
  const int N = h->N, D = h->D;
  const int rc = egp_ensure_factor(h, hyper, Lh);
  if (rc != GPT_OK) {
    nan_fill(fmu, Ntest);
    nan_fill(fs2, Ntest);
    nan_fill(lp, Ntest);
    return rc;
  }
  const EgpHyp H = egp_hyp(hyper, Lh, D);
  hipStream_t st = nullptr;
  const int64_t want = chunk == 0 ? kEgpChunk : std::min<int64_t>(chunk, kEgpChunkMax);
  const int cw = (int)std::min<int64_t>(want, Ntest);
  GPT_HIPCHK(h->Ks.reserve((size_t)N, (size_t)cw));
  // test inputs, targets and the three outputs on the device for the call
  DevMem xmem;
  TestBuffers T;
  GPT_HIPCHK(xmem.alloc<double>((size_t)Ntest * D));
  GPT_HIPCHK(T.alloc((size_t)Ntest, lp != nullptr));
  double *dX = xmem.as<double>(), *dy = T.y, *dmu = T.mu, *dv = T.v, *dlp = T.lp;
  GPT_HIPCHK(hipMemcpyAsync(dX, Xtest, 8 * (size_t)Ntest * D, hipMemcpyHostToDevice, st));
  if (lp) GPT_HIPCHK(hipMemcpyAsync(dy, ytest, 8 * (size_t)Ntest, hipMemcpyHostToDevice, st));
  for (int64_t c0 = 0; c0 < Ntest; c0 += cw) {
    const int nc = (int)std::min<int64_t>(cw, Ntest - c0);
    hipLaunchKernelGGL(egp_cross_kernel, dim3((N + 63) / 64, (nc + 15) / 16), dim3(256), 0, st,
                       h->X, N, dX, (long long)Ntest, (long long)c0, nc, H, h->Ks.p);
    hipLaunchKernelGGL(egp_pred_kernel, dim3((nc + 3) / 4), dim3(256), 0, st, h->Ks.p, N, nc,
                       h->alpha, 0, H.sig2, H.s2, (const double*)nullptr, dmu + c0, dv + c0,
                       (double*)nullptr);
    GPT_HIPCHK(egp_trsm(h->A, N, h->Ks.p, nc, false, st));
    hipLaunchKernelGGL(egp_pred_kernel, dim3((nc + 3) / 4), dim3(256), 0, st, h->Ks.p, N, nc,
                       h->alpha, 1, H.sig2, H.s2, lp ? dy + c0 : (const double*)nullptr, dmu + c0,
                       dv + c0, lp ? dlp + c0 : (double*)nullptr);
    GPT_HIPCHK(hipGetLastError());
  }
  GPT_HIPCHK(T.download(fmu, fs2, lp, st));
  GPT_HIPCHK(hipStreamSynchronize(st));
  return GPT_OK;
}

// ------------------------------------------------------------------------------ function draws
static bool egp_draw_ok(double jitter, int64_t S, int64_t Smin) {
  if (!(jitter >= 0.0) || !std::isfinite(jitter)) {
    set_error("exact GP draw: jitter must be >= 0 and finite"); return false;
  }
  if (S < Smin || S > kGpdSMax) {
    set_error(Smin ? "exact GP draw: S must be in 1..4096"
                   : "exact GP draw: S must be in 0..4096, and in 1..4096 with F");
    return false;
  }
  return true;
}

static bool egp_post_ok(const void* Xtest, int64_t Ntest, double jitter, int32_t observed,
                        int64_t S, const void* fmu, const void* F, const void* cov) {
  if (!egp_draw_ok(jitter, S, F ? 1 : 0)) return false;
  if (Ntest < 1 || Ntest > kGpdTestMax) {
    set_error("exact GP draw: Ntest must be in 1..8192"); return false;
  }
  if (observed != 0 && observed != 1) {
    set_error("exact GP draw: observed must be 0 or 1"); return false;
  }
  if (!fmu && !F && !cov) { set_error("exact GP draw: no output asked for"); return false; }
  if (!Xtest) { set_error("exact GP draw: null test input"); return false; }
  return true;
}

// GPrand (GaussianProcess.jl:66-80) at the handle's X: F (N, S) = L·Z, L·Lᵀ = K + jitter·I.  The
// factor goes where the handle keeps that of K + σ²I, which the call therefore invalidates.
extern "C" int gpt_egp_draw_prior(gpt_egp* h, const double* hyper, int64_t Lh, double jitter,
                                  int64_t S, uint64_t seed, const double* Zin, double* F,
                                  double* Zout) {
  if (!egp_draw_ok(jitter, S, 1)) return GPT_ERR_BAD_DIMS;
  if (!h || !F) { set_error("exact GP draw: null handle or output"); return GPT_ERR_BAD_DIMS; }
  if (!egp_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  const int N = h->N, nblk = (N + 63) / 64;
  EgpHyp H = egp_hyp(hyper, Lh, h->D);
  H.s2 = jitter;                                        // GPrand adds the jitter alone
  hipStream_t st = nullptr;
  h->factor.clear();
  DevSet tmp;
  double *dZ = nullptr, *dF = nullptr;
  const size_t NS = (size_t)N * S;
  GPT_HIPCHK(tmp.alloc(&dZ, NS));
  GPT_HIPCHK(tmp.alloc(&dF, NS));
  GpdTimer tm(st);
  GPT_HIPCHK(hipMemsetAsync(h->status, 0, 16, st));
  GPT_HIPCHK(gpd_normals(dZ, N, (int)S, seed, kGpdPrior, Zin, st));
  tm.mark(0);
  hipLaunchKernelGGL(egp_build_kernel, dim3(nblk, nblk), dim3(256), 0, st, h->X, N, H, h->A);
  GPT_HIPCHK(hipGetLastError());
  tm.mark(1);
  GPT_HIPCHK(egp_chol(h->A, N, h->status, st));
  tm.mark(4);
  GPT_HIPCHK(gpd_trimm(h->A, (size_t)N, N, false, dZ, (int)S, nullptr, 1.0, dF, st));
  tm.mark(5);
  int32_t bad = 0;
  GPT_HIPCHK(hipMemcpyAsync(&bad, h->status, 4, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipMemcpyAsync(F, dF, 8 * NS, hipMemcpyDeviceToHost, st));
  if (Zout) GPT_HIPCHK(hipMemcpyAsync(Zout, dZ, 8 * NS, hipMemcpyDeviceToHost, st));
  GPT_HIPCHK(hipStreamSynchronize(st));
  tm.read();
  if (bad) {
    nan_fill(F, (int64_t)NS);
    nan_fill(Zout, (int64_t)NS);
    set_error("exact GP draw: K + jitter*I is not positive definite (PosDefException)");
    return GPT_ERR_NOT_SPD;
  }
  return GPT_OK;
}

// GPpost + GPrand (GaussianProcess.jl:82-122): the joint posterior at Xtest (Ntest, D) on the
// factor of K + σ²I, fmu by gpt_egp_predict's kernels, Σ = K** − VᵀV with V = L⁻¹Ks, and
// F (Ntest, S) = fmu·1ᵀ + L_Σ·Z, L_Σ·L_Σᵀ = Σ + (jitter [+ σ²])·I.  cov is Σ alone.
extern "C" int gpt_egp_draw_posterior(gpt_egp* h, const double* hyper, int64_t Lh,
                                      const double* Xtest, int64_t Ntest, double jitter,
                                      int32_t observed, int64_t S, uint64_t seed,
                                      const double* Zin, double* fmu, double* F, double* cov,
                                      double* Zout) {
  if (!egp_post_ok(Xtest, Ntest, jitter, observed, S, fmu, F, cov)) return GPT_ERR_BAD_DIMS;
  if (!h) { set_error("exact GP draw: null handle"); return GPT_ERR_BAD_DIMS; }
  if (!egp_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  const int N = h->N, D = h->D, Nt = (int)Ntest, Sd = F ? (int)S : 0;
  const size_t TS = (size_t)Nt * Sd, TT = (size_t)Nt * Nt;
  auto nan_all = [&]() {
    nan_fill(fmu, Nt);
    nan_fill(F, (int64_t)TS);
    nan_fill(cov, (int64_t)TT);
    if (F) nan_fill(Zout, (int64_t)TS);
  };
  const int rc = egp_ensure_factor(h, hyper, Lh);
  if (rc != GPT_OK) { nan_all(); return rc; }
  const EgpHyp H = egp_hyp(hyper, Lh, D);
  hipStream_t st = nullptr;
  GPT_HIPCHK(h->Ks.reserve((size_t)N, (size_t)Nt));
  DevSet tmp;
  double *dX = nullptr, *dmu = nullptr, *dSig = nullptr, *dcov = nullptr, *dZ = nullptr,
         *dF = nullptr;
  GPT_HIPCHK(tmp.alloc(&dX, (size_t)Nt * D));
  GPT_HIPCHK(tmp.alloc(&dmu, (size_t)Nt));
  if (F) {
    GPT_HIPCHK(tmp.alloc(&dSig, TT));
    GPT_HIPCHK(tmp.alloc(&dZ, TS));
    GPT_HIPCHK(tmp.alloc(&dF, TS));
  }
  if (cov) GPT_HIPCHK(tmp.alloc(&dcov, TT));
  GpdTimer tm(st);
  GPT_HIPCHK(hipMemsetAsync(h->status, 0, 16, st));
  GPT_HIPCHK(hipMemcpyAsync(dX, Xtest, 8 * (size_t)Nt * D, hipMemcpyHostToDevice, st));
  if (F) GPT_HIPCHK(gpd_normals(dZ, Nt, Sd, seed, kGpdPosterior, Zin, st));
  tm.mark(0);
  hipLaunchKernelGGL(egp_cross_kernel, dim3((N + 63) / 64, (Nt + 15) / 16), dim3(256), 0, st, h->X,
                     N, dX, (long long)Nt, 0LL, Nt, H, h->Ks.p);
  hipLaunchKernelGGL(egp_pred_kernel, dim3((Nt + 3) / 4), dim3(256), 0, st, h->Ks.p, N, Nt, h->alpha,
                     0, H.sig2, H.s2, (const double*)nullptr, dmu, (double*)nullptr,
                     (double*)nullptr);
  GPT_HIPCHK(hipGetLastError());
  tm.mark(1);
  if (F || cov) {
    GPT_HIPCHK(egp_trsm(h->A, N, h->Ks.p, Nt, false, st));
    tm.mark(2);
    GPT_HIPCHK(gpd_postcov(h->Ks.p, N, dX, Nt, H, jitter + (observed ? H.s2 : 0.0), dSig, dcov, st));
    tm.mark(3);
  }
  if (F) {
    GPT_HIPCHK(egp_chol(dSig, Nt, h->status + 1, st));
    tm.mark(4);
    GPT_HIPCHK(gpd_trimm(dSig, (size_t)Nt, Nt, false, dZ, Sd, dmu, 1.0, dF, st));
    tm.mark(5);
  }
  int32_t bad[2] = {0, 0};
  GPT_HIPCHK(hipMemcpyAsync(bad, h->status, 8, hipMemcpyDeviceToHost, st));
  if (fmu) GPT_HIPCHK(hipMemcpyAsync(fmu, dmu, 8 * (size_t)Nt, hipMemcpyDeviceToHost, st));
  if (cov) GPT_HIPCHK(hipMemcpyAsync(cov, dcov, 8 * TT, hipMemcpyDeviceToHost, st));
  if (F) {
    GPT_HIPCHK(hipMemcpyAsync(F, dF, 8 * TS, hipMemcpyDeviceToHost, st));
    if (Zout) GPT_HIPCHK(hipMemcpyAsync(Zout, dZ, 8 * TS, hipMemcpyDeviceToHost, st));
  }
  GPT_HIPCHK(hipStreamSynchronize(st));
  tm.read();
  if (bad[1]) {
    nan_all();
    set_error(observed ? "exact GP draw: the posterior covariance + (jitter + signal_var)*I is "
                         "not positive definite (PosDefException)"
                       : "exact GP draw: the posterior covariance + jitter*I is not positive "
                         "definite (PosDefException)");
    return GPT_ERR_NOT_SPD;
  }
  return GPT_OK;
}

// One-shot GPrand: create (with targets of zero, which no draw reads), draw, destroy.
extern "C" int gpt_gp_rand(const double* X, int64_t N, int64_t D, const double* hyper, int64_t Lh,
                           double jitter, int64_t S, uint64_t seed, double* F) {
  if (!egp_dims_ok(X, N, D, X) || !egp_hyper_ok(hyper, Lh, D) || !egp_draw_ok(jitter, S, 1))
    return GPT_ERR_BAD_DIMS;
  if (!F) { set_error("exact GP draw: null output"); return GPT_ERR_BAD_DIMS; }
  const std::vector<double> y((size_t)N, 0.0);
  return egp_one_shot(X, N, D, y.data(), [&](gpt_egp* h) {
    return gpt_egp_draw_prior(h, hyper, Lh, jitter, S, seed, nullptr, F, nullptr);
  });
}

// One-shot GPpost + GPrand: create, gpt_egp_draw_posterior, destroy.
extern "C" int gpt_gp_post_rand(const double* X, int64_t N, int64_t D, const double* y,
                                const double* hyper, int64_t Lh, const double* Xtest,
                                int64_t Ntest, double jitter, int32_t observed, int64_t S,
                                uint64_t seed, const double* Zin, double* fmu, double* F,
                                double* cov) {
  if (!egp_dims_ok(X, N, D, y) || !egp_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  if (!egp_post_ok(Xtest, Ntest, jitter, observed, S, fmu, F, cov)) return GPT_ERR_BAD_DIMS;
  return egp_one_shot(X, N, D, y, [&](gpt_egp* h) {
    return gpt_egp_draw_posterior(h, hyper, Lh, Xtest, Ntest, jitter, observed, S, seed, Zin, fmu,
                                  F, cov, nullptr);
  });
}

extern "C" int gpt_gp_nlogmarginal(const double* X, int64_t N, int64_t D, const double* y,
                                   const double* hyper, int64_t Lh, int64_t want_grad,
                                   double* nlml_out, double* grad_out) {
  if (!egp_dims_ok(X, N, D, y) || !egp_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  if (!nlml_out || (want_grad && !grad_out)) {
    set_error("exact GP: null output"); return GPT_ERR_BAD_DIMS;
  }
  return egp_one_shot(X, N, D, y, [&](gpt_egp* h) {
    return gpt_egp_eval(h, hyper, Lh, want_grad ? 1 : 0, nlml_out, grad_out, nullptr);
  });
}

extern "C" int gpt_gp_predict(const double* X, int64_t N, int64_t D, const double* y,
                              const double* hyper, int64_t Lh, const double* Xtest, int64_t Ntest,
                              const double* ytest, double* fmu, double* fs2, double* lp) {
  if (!egp_dims_ok(X, N, D, y) || !egp_hyper_ok(hyper, Lh, D) ||
      !test_args_ok("exact GP", Xtest, Ntest, ytest, 0, fmu, fs2, lp))
    return GPT_ERR_BAD_DIMS;
  return egp_one_shot(X, N, D, y, [&](gpt_egp* h) {
    return gpt_egp_predict(h, hyper, Lh, Xtest, Ntest, ytest, 0, fmu, fs2, lp);
  });
}
