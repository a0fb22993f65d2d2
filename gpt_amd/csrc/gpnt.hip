// Full-theta regression on the device: sibling GPNT_SGLD chains (GPT_SGLD.jl:809-847), one
// workgroup per chain with theta in LDS for a launch of up to one epoch's steps.  The evaluation
// of stored samples reuses nt_scores_kernel (cls.hip) and mean_sse_kernel (pred.hip).
#include "gpt_internal.h"
#include "theta_chain.h"

namespace gpt {

// LDS of gpnt_chain_kernel: theta, the batch's row numbers, targets and residuals, a flag per
// wave, and after them `rows` staged feature rows of n doubles.  mb = min(m, N) is the longest
// batch.  rows = mb: the whole batch in one group; 0 < rows < mb: row groups (a multiple of the
// waves where more than that fit); 0: the second pass reads the rows from memory again.  A group
// keeps one wave busy per row, so groups of fewer than half the waves' rows are not worth the
// single read (4 rows per group are 7 % faster than none, 2 rows 1.4x slower, 1 row
// 2.5x-3.3x slower): then, as when not even one row fits beside theta, nothing is staged.
// rows_cap >= 0 (GPTSGLD_GPNT_ROWS) asks for min(rows_cap, what fits) rows whatever that rule says.
constexpr int kGpntMinRows = kNW / 2;
GpntLayout gpnt_layout(int n, int N, int m, int rows_cap) {
  GpntLayout L;
  const int mb = m < N ? m : N;
  size_t o = 0;
  L.o_theta = o; o = al16(o + 8 * (size_t)n);
  L.o_idx = o;   o = al16(o + 4 * (size_t)mb);
  L.o_y = o;     o = al16(o + 8 * (size_t)mb);
  L.o_res = o;   o = al16(o + 8 * (size_t)mb);
  L.o_flag = o;  o = al16(o + 4 * (size_t)kNW);
  L.o_phi = o;
  L.base = o;
  const size_t row = 8 * (size_t)n;
  long long rows = o < (size_t)kMaxLds ? (long long)(((size_t)kMaxLds - o) / row) : 0;
  if (rows >= mb) rows = mb;
  else if (rows > kNW) rows -= rows % kNW;
  if (rows_cap >= 0) rows = rows < rows_cap ? rows : rows_cap;
  else if (rows < mb && rows < kGpntMinRows) rows = 0;
  L.rows = (int)rows;
  L.groups = L.rows ? (mb + L.rows - 1) / L.rows : 0;
  L.bytes = o + row * (size_t)L.rows;
  return L;
}

// One workgroup per chain runs steps t0 .. t0+nsteps-1 (0-based, within one epoch) with theta in
// LDS; theta goes to HBM on store steps and at the end of the launch.  Per step (:826-843):
//   res_i = y_i − φ_iᵀθ      one wave per batch row, lanes over j (one fma chain per lane in j
//                            order, then wave_sum): the same sum whatever the grouping,
//   g_j = Σ_i φ_ji·res_i     thread per j, one fma chain over i in batch order,
//   θ_j += ε_t/2·(−θ_j/σθ² + (N/B)·g_j/σ²) + sqrt(ε_t)·ξ_j.
// The rows of a group are staged in LDS while their dot products are formed, so each row is read
// from memory once per step; theta does not move inside a step, so a group's residuals are final
// and its share of g is taken from LDS before the next group overwrites it.  PJ > 0: several
// groups per batch, g carried in PJ registers per thread (n <= PJ·kNT).  PJ = 0: one group, or no
// staging at all (L.rows = 0), g formed in one go.  Every exit is taken by the whole workgroup.
constexpr int kGpntU = 32;          // loads of 64 doubles a wave keeps in flight along a row
template <int PJ>
__global__ __launch_bounds__(kNT) void gpnt_chain_kernel(
    const double* __restrict__ phi, const double* __restrict__ y,
    const GpntChain* __restrict__ chains, int n, int N, int m, int nb, long long total,
    double decay_rate, int store_every, long long t0, int nsteps, GpntLayout L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const GpntChain ch = chains[blockIdx.x];
  if (theta_chain_done(t0, total, ch.status)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
  double* theta_l = (double*)(smem + L.o_theta);
  int* idx_l = (int*)(smem + L.o_idx);
  double* yb_l = (double*)(smem + L.o_y);
  double* res_l = (double*)(smem + L.o_res);
  int* flag_l = (int*)(smem + L.o_flag);
  double* phi_l = (double*)(smem + L.o_phi);
  const int G = L.rows;
  for (int j = tid; j < n; j += kNT) theta_l[j] = ch.theta[j];
  const double isg2 = 1.0 / (ch.sigma_theta * ch.sigma_theta);
  const long long tend = min(total, t0 + (long long)nsteps);

  // rows i0 .. i1-1 of the batch: res_l[i], and with `stage` the row into slot i - i0 of phi_l
  auto dots = [&](int i0, int i1, bool stage) {
    for (int i = i0 + wv; i < i1; i += kNW) {
      const double* col = phi + (long long)uni(idx_l[i]) * n;
      double* dst = phi_l + (size_t)(i - i0) * n;
      double acc = 0.0;
      for (int j0 = lane; j0 < n; j0 += 64 * kGpntU) {
        double pv[kGpntU];
#pragma unroll
        for (int u = 0; u < kGpntU; ++u) pv[u] = col[min(j0 + 64 * u, n - 1)];
#pragma unroll
        for (int u = 0; u < kGpntU; ++u) {
          const int j = j0 + 64 * u;
          if (j < n) {
            if (stage) dst[j] = pv[u];
            acc = fma(pv[u], theta_l[j], acc);
          }
        }
      }
      acc = wave_sum(acc);
      if (lane == 0) res_l[i] = yb_l[i] - acc;
    }
  };

  for (long long t = t0; t < tend; ++t) {
    const int32_t* ord;
    const int Bt = theta_batch(ch.order, t, nb, m, N, &ord);
    __syncthreads();                          // theta_l loaded / the step before is finished
    gather_batch(ord, Bt, N, y, idx_l, yb_l);
    __syncthreads();
    const ThetaStepSize S = theta_step_size(ch.eps_theta, t, decay_rate, N, Bt);
    const double eps = S.eps, sq = S.sq, cN = S.cN;
    double* out = theta_store_slot(ch.store, t, store_every, (size_t)n);
    bool bad = false;
    auto move = [&](int j, double g) {
      const double th = theta_l[j];
      const double grad = -th * isg2 + cN * g / ch.signal_var;
      const double nt = th + (eps * grad / 2 +
                              sq * normal_at(ch.seed, (uint32_t)j, (uint32_t)t, kThetaNoise, 0));
      theta_l[j] = nt;
      if (out) out[j] = nt;
      bad |= (nt != nt);
    };
    if constexpr (PJ > 0) {
      double g[PJ];
#pragma unroll
      for (int p = 0; p < PJ; ++p) g[p] = 0.0;
      for (int i0 = 0; i0 < Bt; i0 += G) {
        const int cnt = min(G, Bt - i0);
        dots(i0, i0 + cnt, true);
        __syncthreads();
        // i outside, the thread's PJ columns inside: PJ independent chains, each still in i order
        // (a column past n reads column n-1 and is never used)
#pragma unroll 1
        for (int i = 0; i < cnt; ++i) {
          const double r = res_l[i0 + i];
          const double* row = phi_l + (size_t)i * n;
#pragma unroll
          for (int p = 0; p < PJ; ++p) g[p] = fma(row[min(tid + kNT * p, n - 1)], r, g[p]);
        }
        __syncthreads();                      // the group's slots are free again
      }
      // through the first slot, free again, so that the move is one loop over the thread's own j
#pragma unroll
      for (int p = 0; p < PJ; ++p)
        if (tid + kNT * p < n) phi_l[tid + kNT * p] = g[p];
      for (int j = tid; j < n; j += kNT) move(j, phi_l[j]);
    } else {
      dots(0, Bt, G > 0);
      __syncthreads();
      for (int j = tid; j < n; j += kNT) {
        double g = 0.0;
        if (G > 0) {
          for (int i = 0; i < Bt; ++i) g = fma(phi_l[(size_t)i * n + j], res_l[i], g);
        } else {
          for (int i0 = 0; i0 < Bt; i0 += 8) {
            double pv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) pv[u] = phi[(long long)idx_l[min(i0 + u, Bt - 1)] * n + j];
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (i0 + u < Bt) g = fma(pv[u], res_l[i0 + u], g);
          }
        }
        move(j, g);
      }
    }
    // theta_chain_nan, written out: through the helper this kernel runs 0.3-1.4 % slower
    const int wbad = __ballot(bad) != 0 ? 1 : 0;
    if (lane == 0) flag_l[wv] = wbad;
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int w2 = 0; w2 < kNW; ++w2) any |= flag_l[w2];
    if (any) {
      if (tid == 0)
        __hip_atomic_store(ch.status, GPT_ERR_NAN_THETA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
  __syncthreads();
  for (int j = tid; j < n; j += kNT) ch.theta[j] = theta_l[j];
}

// The register carry of the grouped route: n <= PJ·kNT for the smallest listed PJ.  The largest
// covers every n at which a row still fits beside theta (2·8·n <= 160 KiB).
using GpntCarries = IntList<1, 2, 4, 8, 12, 16, 20>;
template <int... Vs> static int gpnt_carry(IntList<Vs...>, int n) {
  int pj = -1;
  (void)((n <= Vs * kNT && ((pj = Vs), true)) || ...);
  return pj;
}

hipError_t launch_gpnt_chain(const double* phi, const double* y, const GpntChain* chains,
                             int nchains, int n, int N, int m, int nb, long long total,
                             double decay_rate, int store_every, long long t0, int nsteps,
                             const GpntLayout& L, hipStream_t st) {
  if (L.base > (size_t)kMaxLds || L.bytes > (size_t)kMaxLds || nchains < 1 || store_every < 1)
    return hipErrorInvalidValue;
  const int pj = L.groups > 1 ? gpnt_carry(GpntCarries{}, n) : 0;
  return with_value(IntList<0, 1, 2, 4, 8, 12, 16, 20>{}, pj, [&](auto PJ) {
    return launch_lds_over_64k<gpnt_chain_kernel<PJ>>(
        kMaxLds, dim3(nchains), dim3(kNT), L.bytes, st, phi, y, chains, n, N, m, nb, total,
        decay_rate, store_every, t0, nsteps, L);
  });
}

}  // namespace gpt
