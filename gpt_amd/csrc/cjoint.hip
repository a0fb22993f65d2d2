// Joint likelihood of the full-theta softmax classifier, −log p(y, θ; h), and its gradient with
// respect to θ and h = [length_scale; sigma_RBF] (neglogjointlkhd / gradneglogjointlkhd,
// ImageExperiment.jl:135-204; the objective of GPNT_hyperparameters_ng, GPT_SGLD.jl:1005-1063)
// for MI355X (gfx950).  DESIGN §6e.
//
// f = Zt·Xᵀ + b, Zt = Z ./ ℓ, c = sqrt(2/n)·σ, φ = c·cos f, S = c·sin f, s = θᵀφ (C × N),
// R = softmax(s) − onehot(y):
//   value = Σ_i (lse_i − s[y_i, i]) + ‖θ‖²/2,           ∂/∂θ = φ·Rᵀ + θ,
//   ∂/∂ℓ_k = (1/ℓ_k) Σ_j Zt[j,k]·((S ∘ θR)·X)[j,k],     ∂/∂σ = (Σ R ∘ s)/σ.
// The reference forms gradfeatureNotensor's n × N × D array; here a workgroup forms φ and S of a
// tile of TI data columns once, in LDS, and every contraction reads that tile.  All fp64, no
// atomics on doubles, every sum in a fixed order that depends on the shape alone.
#include <cfloat>

#include "device_util.h"

namespace gpt {

constexpr size_t kCjLds = kMaxLds;

// LDS of cjoint_eval_kernel.  Fixed part: the scores / residual of the tile sr[ii][CC], the tile's
// rows of X padded to 16 (X[ii][16]), 1/ℓ (16) and the workgroup sum's scratch.  Then the tile:
// φ and S, n × TI doubles each, column ii at ii·n.  TI is the largest of 32, 16, 8 for which
// fixed + 16·n·TI bytes fit the 160 KB (n = 1024: 8), a function of n and C alone.  θ (n × CC, the
// columns past C zero) follows the tile when its 8·n·CC bytes still fit; otherwise the kernel
// reads θ through L2 (n = 330, C = 32: the tile takes 84 KB of TI = 16 and θ another 84 KB).
CjLayout cjoint_layout(int n, long long N, int C) {
  CjLayout L;
  L.CC = C <= 2 ? 2 : (C <= 4 ? 4 : (C <= 8 ? 8 : (C <= 16 ? 16 : 32)));
  for (L.TI = 32;; L.TI /= 2) {
    size_t o = 0;
    L.o_sr = o;  o = al16(o + 8 * (size_t)L.CC * L.TI);
    L.o_X = o;   o = al16(o + 8 * (size_t)16 * L.TI);
    L.o_inv = o; o = al16(o + 8 * (size_t)16);
    L.o_red = o; o = al16(o + 8 * (size_t)kNW);
    L.o_phi = o; o = al16(o + 8 * (size_t)n * L.TI);
    L.o_S = o;   o = al16(o + 8 * (size_t)n * L.TI);
    L.o_theta = o;
    L.bytes = o;
    if (o <= kCjLds || L.TI == 8) break;
  }
  const size_t with_theta = al16(L.bytes + 8 * (size_t)n * L.CC);
  L.theta_lds = with_theta <= kCjLds ? 1 : 0;
  if (L.theta_lds) L.bytes = with_theta;
  L.ntiles = (N + L.TI - 1) / L.TI;
  L.nblk = (int)(L.ntiles < kCjMaxBlocks ? L.ntiles : kCjMaxBlocks);
  return L;
}

// A workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... in order.  Per tile:
//   A  φ, S of the tile into LDS, the argument formed exactly as feature_notensor_kernel forms it:
//      a thread owns a feature j with Zt[j, :] and b[j] in registers and walks a group of columns;
//   B  scores: a wave owns a unit of CGS classes × 4 columns, lanes over j, the lane sums combined
//      by Butterfly's fixed exchange pattern;
//   softmax: one thread per column — max-subtracted lse, the value and σ terms, R in place;
//   C  φ·Rᵀ: a thread owns (CGS classes, j), columns in order, added to the workgroup's partial;
//   D  (S ∘ θR)·X: a thread owns j, θ[j, :] in registers, columns in order, added to the partial.
// A partial entry has one owner thread, so its read-modify-write needs no atomic (the old value is
// loaded before the column loop, which hides the load); columns past N
// have X = 0 and R = 0 and add exact zeros.
template <int CC, int MODE>
__global__ __launch_bounds__(kNT) void cjoint_eval_kernel(const CjArgs A, const CjLayout L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (A.status && __hip_atomic_load(A.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  constexpr bool kNeedS = MODE == kCjFull || MODE == kCjFeatures;
  constexpr bool kLik = MODE == kCjValue || MODE == kCjTheta || MODE == kCjFull;
  constexpr bool kGradTheta = MODE == kCjTheta || MODE == kCjFull;
  constexpr int CGS = CC < 4 ? CC : 4;        // classes of a unit
  constexpr int NCG = CC / CGS;
  const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
  const int n = A.n, C = A.C, D = A.D, TI = L.TI;
  const long long N = A.N;
  double* sr_l = (double*)(smem + L.o_sr);
  double* X_l = (double*)(smem + L.o_X);
  double* inv_l = (double*)(smem + L.o_inv);
  double* red_l = (double*)(smem + L.o_red);
  double* phi_l = (double*)(smem + L.o_phi);
  double* S_l = (double*)(smem + L.o_S);
  double* theta_l = (double*)(smem + L.o_theta);
  const bool tl = L.theta_lds != 0;
  if (tid < 16) inv_l[tid] = tid < D ? 1.0 / A.ls[tid] : 0.0;
  if (tl && MODE != kCjFeatures)
    for (int e = tid; e < n * CC; e += kNT) theta_l[e] = e < n * C ? A.theta[e] : 0.0;
  const int NP = ((n + 63) / 64) * 64;
  // phase A: NPA threads (whole waves) over j, GA groups of them over the tile's columns
  const int NPA = NP < kNT ? NP : kNT, GA = kNT / NPA;
  const int ga = tid / NPA, ja = tid - ga * NPA;
  const FastDiv fdnp = fast_div(NP);          // fdiv(e, ·) is exact: e·NP < 8·NP² <= 2²³
  double v_acc = 0.0, r_acc = 0.0;            // thread ii < TI: its columns' terms, tiles in order
  for (long long tile = blockIdx.x; tile < L.ntiles; tile += gridDim.x) {
    const long long i0 = tile * TI;
    const bool first = tile == (long long)blockIdx.x;
    __syncthreads();                          // the tile before is done with X_l, the tile and sr_l
    for (int e = tid; e < 16 * TI; e += kNT) {
      const int k = e / TI, ii = e - k * TI;
      const long long i = i0 + ii;
      X_l[ii * 16 + k] = (k < D && i < N) ? A.X[i + N * k] : 0.0;
    }
    __syncthreads();
    if (ga < GA) {
      for (int j = ja; j < n; j += NPA) {
        double zt[16];
#pragma unroll
        for (int k = 0; k < 16; ++k)
          zt[k] = k < D ? __dmul_rn(A.Z[j + (size_t)n * k], inv_l[k]) : 0.0;
        const double bj = A.b[j];
        for (int ii = ga; ii < TI; ii += GA) {
          const double* xr = X_l + 16 * ii;
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 16; ++k)
            if (k < D) s = __dadd_rn(s, __dmul_rn(xr[k], zt[k]));
          const double f = __dadd_rn(s, bj);
          phi_l[ii * n + j] = __dmul_rn(A.c, cos(f));
          if constexpr (kNeedS) S_l[ii * n + j] = __dmul_rn(A.c, sin(f));
        }
      }
    }
    __syncthreads();
    if constexpr (MODE == kCjFeatures) continue;

    const int units = NCG * (TI / 4);
    for (int u = wv; u < units; u += kNW) {
      const int cg = u % NCG, q0 = (u / NCG) * 4, c0 = cg * CGS;
      double acc[CGS * 4];
#pragma unroll
      for (int x = 0; x < CGS * 4; ++x) acc[x] = 0.0;
      for (int j = lane; j < n; j += 64) {
        double th[CGS], ph[4];
#pragma unroll
        for (int a = 0; a < CGS; ++a) {
          const int c = c0 + a;
          th[a] = tl ? theta_l[c * n + j] : (c < C ? A.theta[(size_t)c * n + j] : 0.0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) ph[q] = phi_l[(q0 + q) * n + j];
#pragma unroll
        for (int a = 0; a < CGS; ++a)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[a * 4 + q] = fma(ph[q], th[a], acc[a * 4 + q]);
      }
      Butterfly<CGS * 4>::run(acc, lane);     // lane λ: the total of value λ >> SH
      constexpr int SH = CGS == 4 ? 2 : 3;
      if ((lane & ((1 << SH) - 1)) == 0) {
        const int v = lane >> SH, a = v >> 2, q = v & 3;
        sr_l[(q0 + q) * CC + c0 + a] = acc[0];
      }
    }
    __syncthreads();

    if constexpr (MODE == kCjScores) {
      for (int e = tid; e < C * TI; e += kNT) {
        const int c = e / TI, ii = e - c * TI;
        const long long i = i0 + ii;
        if (i < N) A.scores[i + N * c] = sr_l[ii * CC + c];
      }
      continue;
    }

    if constexpr (kLik) {
      if (tid < TI) {
        const long long i = i0 + tid;
        double* col = sr_l + tid * CC;
        if (i < N) {
          double a = col[0];
          for (int c = 1; c < C; ++c) a = fmax(a, col[c]);
          double s = 0.0;
          for (int c = 0; c < C; ++c) s += exp(col[c] - a);
          const double lse = a + log(s);
          const int yi = min(max(A.y0[i], 0), C - 1);      // labels are checked on the host
          const double nl = lse - col[yi];
          v_acc += nl;
          if constexpr (kGradTheta) {
            double rs = 0.0;
            for (int c = 0; c < C; ++c) {
              const double sc = col[c];
              const double r = exp(sc - lse) - (c == yi ? 1.0 : 0.0);
              rs = fma(r, sc, rs);
              col[c] = r;
            }
            r_acc += rs;
          }
        } else {
          for (int c = 0; c < C; ++c) col[c] = 0.0;
        }
      }
    }
    if constexpr (kGradTheta) {
      __syncthreads();
      double* pth = A.part_theta + (size_t)blockIdx.x * n * C;
      for (int e = tid; e < NP * NCG; e += kNT) {
        const int cg = fdiv(e, fdnp), j = e - cg * NP;     // cg is uniform over a wave
        if (j >= n) continue;
        const int c0 = cg * CGS;
        double g[CGS], old[CGS];
#pragma unroll
        for (int a = 0; a < CGS; ++a) {                    // the loads fly during the column loop
          g[a] = 0.0;
          old[a] = (!first && c0 + a < C) ? pth[(size_t)(c0 + a) * n + j] : 0.0;
        }
        for (int ii = 0; ii < TI; ++ii) {
          const double p = phi_l[ii * n + j];
          const double* r = sr_l + ii * CC + c0;           // read by broadcast
#pragma unroll
          for (int a = 0; a < CGS; ++a) g[a] = fma(p, r[a], g[a]);
        }
#pragma unroll
        for (int a = 0; a < CGS; ++a)
          if (c0 + a < C) pth[(size_t)(c0 + a) * n + j] = first ? g[a] : old[a] + g[a];
      }
    }
    if constexpr (MODE == kCjFull) {
      double* ptx = A.part_tx + (size_t)blockIdx.x * n * D;
      for (int j = tid; j < n; j += kNT) {
        double th[CC], acc[16], old[16];
#pragma unroll
        for (int c = 0; c < CC; ++c)
          th[c] = tl ? theta_l[c * n + j] : (c < C ? A.theta[(size_t)c * n + j] : 0.0);
#pragma unroll
        for (int k = 0; k < 16; ++k) {                     // the loads fly during the column loop
          acc[k] = 0.0;
          old[k] = (!first && k < D) ? ptx[(size_t)k * n + j] : 0.0;
        }
        for (int ii = 0; ii < TI; ++ii) {
          const double* r = sr_l + ii * CC;                // entries past C are exact zeros
          double g = 0.0;
#pragma unroll
          for (int c = 0; c < CC; ++c) g = fma(th[c], r[c], g);
          const double t = S_l[ii * n + j] * g;
          const double* xr = X_l + 16 * ii;
#pragma unroll
          for (int k = 0; k < 16; ++k)
            if (k < D) acc[k] = fma(t, xr[k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k < D) ptx[(size_t)k * n + j] = first ? acc[k] : old[k] + acc[k];
      }
    }
  }
  if constexpr (kLik) {
    __syncthreads();
    const double vs = blk_sum(v_acc, red_l), rs = blk_sum(r_acc, red_l);
    if (tid == 0) {
      A.part_sc[2 * blockIdx.x] = vs;
      A.part_sc[2 * blockIdx.x + 1] = rs;
    }
  }
}

// The partials in workgroup order.  Workgroup 0: out[0] = Σ value partials + ‖θ‖²/2 and out[1] =
// (Σ σ partials)/σ.  With `full`, workgroup 1 + k: out[2 + k] = (1/ℓ_k) Σ_j Zt[j,k]·Σ_b tx[b][j][k]
// (nlml_finish_kernel's form), and the workgroups after them: out[2 + D + e] = Σ_b pθ[b][e] + θ[e].
__global__ __launch_bounds__(kNT) void cjoint_finish_kernel(const CjArgs A, int nblk, double sigma,
                                                            double* __restrict__ out) {
  __shared__ double red[kNW];
  const int n = A.n, D = A.D, tid = threadIdx.x;
  const size_t nC = (size_t)n * A.C;
  if (blockIdx.x == 0) {
    double tt = 0.0;
    for (size_t e = tid; e < nC; e += kNT) tt = fma(A.theta[e], A.theta[e], tt);
    const double t2 = blk_sum(tt, red);
    if (tid == 0) {
      double v = 0.0, r = 0.0;
      for (int b = 0; b < nblk; ++b) {
        v += A.part_sc[2 * b];
        r += A.part_sc[2 * b + 1];
      }
      out[0] = __dadd_rn(v, __dmul_rn(0.5, t2));
      out[1] = r / sigma;
    }
  } else if ((int)blockIdx.x <= D) {
    const int k = blockIdx.x - 1;
    const double inv = 1.0 / A.ls[k];
    double s = 0.0;
    for (int j = tid; j < n; j += kNT) {
      double g = 0.0;
      for (int b = 0; b < nblk; ++b) g += A.part_tx[((size_t)b * D + k) * n + j];
      s = fma(__dmul_rn(A.Z[j + (size_t)n * k], inv), g, s);
    }
    const double tot = blk_sum(s, red);
    if (tid == 0) out[2 + k] = tot / A.ls[k];
  } else {
    const size_t e = (size_t)(blockIdx.x - 1 - D) * kNT + tid;
    if (e < nC) {
      double g = 0.0;
      for (int b = 0; b < nblk; ++b) g += A.part_theta[(size_t)b * nC + e];
      out[2 + D + e] = g + A.theta[e];
    }
  }
}

// The Langevin step on the resident θ (GPT_SGLD.jl:1032), one thread per entry; ξ of 0-based step
// t, feature j, class c is normal_at(seed, j, t, kThetaNoise, c), ntc_chain_kernel's contract.
// A θ that turns non-finite sets status, and every later launch of the run returns at once.
__global__ __launch_bounds__(256) void cjoint_update_kernel(const double* __restrict__ part_theta,
                                                            int nblk, double* __restrict__ theta,
                                                            int n, int C, double eps, double sq,
                                                            uint64_t seed, uint32_t t,
                                                            int32_t* __restrict__ status) {
  if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  const size_t nC = (size_t)n * C;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nC) return;
  const int c = (int)(e / n), j = (int)(e - (size_t)c * n);
  double g = 0.0;
  for (int b = 0; b < nblk; ++b) g += part_theta[(size_t)b * nC + e];
  const double th = theta[e];
  const double grad = g + th;
  const double xi = normal_at(seed, (uint32_t)j, t, kThetaNoise, (uint32_t)c);
  const double nt = th - (eps * grad / 2 + sq * xi);
  theta[e] = nt;
  if (!(fabs(nt) <= DBL_MAX))
    __hip_atomic_store(status, GPT_ERR_NAN_THETA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_cjoint_eval(const CjArgs& A, const CjLayout& L, int mode, hipStream_t st) {
  if (A.n < 1 || A.n > 1024 || A.D < 1 || A.D > kDMax || A.C < 1 || A.C > 32 || A.N < 1 ||
      L.bytes > kCjLds || L.nblk < 1 || L.nblk > kCjMaxBlocks)
    return hipErrorInvalidValue;
  using Modes = IntList<kCjValue, kCjTheta, kCjFull, kCjScores, kCjFeatures>;
  return with_value(IntList<2, 4, 8, 16, 32>{}, L.CC, [&](auto CC) {
    return with_value(Modes{}, mode, [&](auto MODE) {
      return launch_lds_over_64k<cjoint_eval_kernel<CC, MODE>>((int)kCjLds, dim3(L.nblk), dim3(kNT),
                                                               L.bytes, st, A, L);
    });
  });
}

hipError_t launch_cjoint_finish(const CjArgs& A, const CjLayout& L, double sigma, bool full,
                                double* out, hipStream_t st) {
  const size_t nC = (size_t)A.n * A.C;
  const unsigned grid = full ? (unsigned)(1 + A.D + (nC + kNT - 1) / kNT) : 1u;
  hipLaunchKernelGGL(cjoint_finish_kernel, dim3(grid), dim3(kNT), 0, st, A, L.nblk, sigma, out);
  return hipGetLastError();
}

hipError_t launch_cjoint_update(const CjArgs& A, const CjLayout& L, double* theta, double eps,
                                uint64_t seed, uint32_t t, int32_t* status, hipStream_t st) {
  const size_t nC = (size_t)A.n * A.C;
  hipLaunchKernelGGL(cjoint_update_kernel, dim3((unsigned)((nC + 255) / 256)), dim3(256), 0, st,
                     A.part_theta, L.nblk, theta, A.n, A.C, eps, std::sqrt(eps), seed, t, status);
  return hipGetLastError();
}

}  // namespace gpt
