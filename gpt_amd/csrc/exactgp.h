// What exactgp.hip, nlml.hip and gpdraw.hip share: the exact GP's kernel function and the launchers
// of the function-draw kernels (gpdraw.hip).
#pragma once
#include "device_util.h"

namespace gpt {

struct EgpHyp {
  double invl[kDMax];   // 1/ℓ_k
  double sig2, s2;      // σ_RBF², σ²
  int D;
};

// k(a, b) for rows ia of Xa (stride sa between dimensions) and ib of Xb
__device__ __forceinline__ double egp_kern(const double* __restrict__ Xa, size_t sa, size_t ia,
                                           const double* __restrict__ Xb, size_t sb, size_t ib,
                                           const EgpHyp& H) {
  double s = 0.0;
  for (int k = 0; k < H.D; ++k) {
    const double d = (Xa[ia + sa * k] - Xb[ib + sb * k]) * H.invl[k];
    s = fma(d, d, s);
  }
  return H.sig2 * exp(-0.5 * s);
}

// ---- gpdraw.hip.  All matrices column-major fp64 on the device.
constexpr int kGpdSMax = 4096;       // draws per call
constexpr int kGpdTestMax = 8192;    // test rows of a joint posterior
enum GpdKind : uint32_t { kGpdPrior = 0, kGpdPosterior = 1, kGpdTheta = 2 };
// The normals of a call, Z (M × S): the caller's Zin (host) when given, else element (i, s) =
// normal_at(seed, i, s, kGpDraw, kind).
hipError_t gpd_normals(double* Z, int M, int S, uint64_t seed, uint32_t kind, const double* Zin,
                       hipStream_t st);
// F (M × S) = mu·1ᵀ + c·T·Z for the triangular T (M × M, leading dimension ld): the lower triangle
// of T when !upper (what lies above it is never read), the upper one otherwise.  mu may be null.
hipError_t gpd_trimm(const double* T, size_t ld, int M, bool upper, const double* Z, int S,
                     const double* mu, double c, double* F, hipStream_t st);
// Σ = K(Xt, Xt) − VᵀV for V (N × Nt, leading dimension N) and Xt (Nt, D): Sig (optional) receives
// the lower 64 × 64 blocks of Σ + d·I, cov (optional) all of Σ.
hipError_t gpd_postcov(const double* V, int N, const double* Xt, int Nt, const EgpHyp& H, double d,
                       double* Sig, double* cov, hipStream_t st);
// Device-event times of the calling thread's last draw call (gpt_gpdraw_last_timing).
constexpr int kGpdPhases = 6;        // noise, assembly, solve, covariance, Cholesky, product
double* gpd_phase_ms();
// Event marks of one draw call: the time between two marks goes to the phase the later one names;
// read() after the stream has drained.
struct GpdTimer {
  static constexpr int kMax = 12;
  hipEvent_t ev[kMax];
  int phase[kMax], n = 0;
  hipStream_t st;
  explicit GpdTimer(hipStream_t s) : st(s) { mark(-1); }
  GpdTimer(const GpdTimer&) = delete;
  GpdTimer& operator=(const GpdTimer&) = delete;
  void mark(int ph) {
    if (n < kMax && hipEventCreate(&ev[n]) == hipSuccess) {
      (void)hipEventRecord(ev[n], st);
      phase[n++] = ph;
    }
  }
  void read() {
    double* ms = gpd_phase_ms();
    for (int q = 0; q < kGpdPhases; ++q) ms[q] = 0.0;
    for (int k = 1; k < n; ++k) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev[k - 1], ev[k]) == hipSuccess && phase[k] >= 0) ms[phase[k]] += t;
    }
  }
  ~GpdTimer() { for (int k = 0; k < n; ++k) (void)hipEventDestroy(ev[k]); }
};

}  // namespace gpt
