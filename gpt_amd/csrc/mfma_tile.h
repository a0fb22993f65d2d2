// The fp64 matrix-core tile loop for GEMMs whose two operands are both contiguous in K
// (pred.hip's stacked-sample phidotU, nlml.hip's gradient, predictive variance and kernel error).
#pragma once
#include "device_util.h"

namespace gpt {

// The 16-byte pair at p, loaded within p's own address space.
__device__ __forceinline__ d2 vec2_of(const double* p) { return *(const d2*)p; }
__device__ __forceinline__ d2 vec2_of(const __attribute__((address_space(1))) double* p) {
  return *(const __attribute__((address_space(1))) d2*)p;
}

// acc[t][u] += Σ_{k < kend} A_t[k]·B_u[k] on v_mfma_f64_16x16x4f64, for one wave's TM × TN tiles of
// 16 × 16.  pa[t] and pb[u] are the lane's own rows: row λ&15 of A tile t and of B tile u, both
// K-contiguous and of length n.  kend <= n, and kend < n only where A's rows are zero from kend on:
// the sum runs in blocks of 16 and stops at the first block end at or past kend, or at n.
// kl = λ>>4.
//
// Lane λ feeds the K pair j0 + 2(λ>>4) + {0,1} of its rows, one 16-B load per row when n is even
// (V2: j is even and the rows are 16-B aligned) and two scalars otherwise; the two halves go to two
// MFMAs (any K order common to A and B is the same sum).  mma runs every accumulator with the even
// K half, then with the odd one: TM·TN >= 4 independent MFMAs between two on one accumulator.
//
// The operand loads are free of branches and selects: the address is clamped in-row (to n − 2 for
// a pair, n − 1 for a scalar), and a lane whose row lies outside the matrix is pointed by the caller
// at a valid row and only feeds outputs that the caller never uses.  So the loaded values go
// straight into the MFMAs, and over the full blocks of 16 two operand sets ping-pong: one step's
// loads are in flight while the other step's MFMAs run.  Only the K tail (j >= n) is zeroed, after
// the loop, and in A alone: B's halves past n are clamped reads of its own row, finite matrix
// entries, and a zero times those adds an exact zero.
//
// Output layout: acc[t][u][reg] = D[row = (λ>>4) + 4·reg][col = λ&15], row ↔ A's rows, col ↔ B's.
template <bool V2, int TM, int TN, class PA, class PB>
__device__ __forceinline__ void mfma_kpair_tile(PA const (&pa)[TM], PB const (&pb)[TN], int n,
                                                int kend, int kl, d4 (&acc)[TM][TN]) {
  auto ld = [&](auto p, int j, double& x0, double& x1) {
    if constexpr (V2) {              // n even: j even, rows 16-B aligned
      const d2 v = vec2_of(p + min(j, n - 2));
      x0 = v[0]; x1 = v[1];
    } else {
      x0 = p[min(j, n - 1)];
      x1 = p[min(j + 1, n - 1)];
    }
  };
  struct Ops { double a0[TM], a1[TM], b0[TN], b1[TN]; };
  auto load = [&](int j, Ops& o) {
#pragma unroll
    for (int t = 0; t < TM; ++t) ld(pa[t], j, o.a0[t], o.a1[t]);
#pragma unroll
    for (int u = 0; u < TN; ++u) ld(pb[u], j, o.b0[u], o.b1[u]);
  };
  auto ktail = [&](int j, Ops& o) {    // zero the A halves past n (one operand suffices)
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      o.a0[t] = j < n ? o.a0[t] : 0.0;
      o.a1[t] = j + 1 < n ? o.a1[t] : 0.0;
    }
  };
  auto mma = [&](const Ops& o) {
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int u = 0; u < TN; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a0[t], o.b0[u], acc[t][u], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int u = 0; u < TN; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a1[t], o.b1[u], acc[t][u], 0, 0, 0);
  };
  // two K steps of 8 per iteration over the full 16-blocks, then the masked tail
  const int nfull = kend & ~15;
  Ops X, Y;
  load(2 * kl, X);
  for (int j0 = 0; j0 < nfull; j0 += 16) {
    load(j0 + 8 + 2 * kl, Y);
    mma(X);
    load(j0 + 16 + 2 * kl, X);
    mma(Y);
  }
  if (nfull < kend) {
    load(nfull + 8 + 2 * kl, Y);
    ktail(nfull + 2 * kl, X);
    ktail(nfull + 8 + 2 * kl, Y);
    mma(X);
    mma(Y);
  }
}

}  // namespace gpt
