// GPT_inf (the Gibbs sampler of the tensor GP) and GPT_GMC from host arrays.
#include <cmath>
#include <cstring>
#include <vector>

#include "host_util.h"

using namespace gpt;

extern "C" int gpt_tgp_gibbs(const double* b, const double* y, int64_t n, int64_t D, int64_t N,
                             int64_t r, int64_t q, double sigma, int64_t num_iterations,
                             int64_t burnin, uint64_t seed, const int32_t* I, double* W_out,
                             double* U_out, int32_t* I_out) {
  if (!b || !y || !W_out || !U_out || n < 1 || D < 1 || N < 1 || q < 1 || burnin < 0 ||
      num_iterations <= burnin || !(sigma > 0)) {
    set_error("bad GPT_inf arguments"); return GPT_ERR_BAD_DIMS;
  }
  if (!rank_supported((int)r)) { set_error("rank r not instantiated (supported: " + ranks_text() + ")"); return GPT_ERR_BAD_DIMS; }
  if (n * r > 8192 || q > 8192 || (double)n * D * N > 2e9) { set_error("dimension too large"); return GPT_ERR_BAD_DIMS; }
  std::vector<int32_t> I0((size_t)q * D);
  if (I) {
    if (!zero_based_I(I, q, D, r, I0)) return GPT_ERR_BAD_DIMS;
  } else {
    for (int64_t e = 0; e < q * D; ++e) {
      const U4 x = philox4x32((uint32_t)e, 0, kTgpI, 0, seed);
      I0[e] = (int32_t)(((uint64_t)x.x * (uint64_t)r) >> 32);
    }
  }
  if (I_out)
    for (int64_t e = 0; e < q * D; ++e) I_out[e] = I0[e] + 1;
  const int64_t nr = n * r, T = num_iterations - burnin;
  std::vector<double> U0((size_t)nr * D);
  const double su = std::sqrt(1.0 / (double)r);
  for (int64_t d = 0; d < D; ++d)
    for (int64_t e = 0; e < nr; ++e) U0[d * nr + e] = su * host_normal(seed, (uint32_t)e, 0, kTgpUInit, (uint32_t)d);
  DevMem db, dy, dI, dU, dW, dUh, dst;
  GPT_HIPCHK(db.upload(b, (size_t)n * D * N));
  GPT_HIPCHK(dy.upload(y, (size_t)N));
  GPT_HIPCHK(dI.upload(I0.data(), I0.size()));
  GPT_HIPCHK(dU.upload(U0.data(), U0.size()));
  GPT_HIPCHK(dW.alloc<double>((size_t)q * T));
  GPT_HIPCHK(dUh.alloc<double>((size_t)nr * D * T));
  GPT_HIPCHK(dst.alloc<int32_t>(1));
  GPT_HIPCHK(dst.zero());
  hipError_t e = tgp_gibbs(db.as<double>(), dy.as<double>(), (int)n, (int)D, N, (int)r, (int)q, sigma,
                           (int)num_iterations, (int)burnin, seed, dI.as<int32_t>(), dU.as<double>(),
                           dW.as<double>(), dUh.as<double>(), dst.as<int32_t>(), nullptr);
  if (e != hipSuccess) return hip_fail(e, "tgp gibbs");
  GPT_HIPCHK(hipStreamSynchronize(nullptr));
  int32_t stt = 0;
  GPT_HIPCHK(dst.download(&stt, 1));
  if (stt) { set_error("PosDefException: Gibbs precision matrix not positive definite"); return GPT_ERR_NOT_SPD; }
  GPT_HIPCHK(dW.download(W_out, (size_t)q * T));
  GPT_HIPCHK(dUh.download(U_out, (size_t)nr * D * T));
  return GPT_OK;
}

extern "C" int gpt_gmc(const double* phi, const double* y, int64_t n, int64_t D, int64_t N,
                       int64_t r, int64_t Q, const int32_t* I, double signal_var, double epsw,
                       double epsU, int64_t burnin, int64_t maxepoch, int64_t L, uint64_t seed,
                       const double* w_init, const double* U_init, double* w_store,
                       double* U_store, double* accept_prob) {
  if (!phi || !y || !I || !w_store || !U_store || !accept_prob || n < 1 || D < 1 || N < 1 ||
      Q < 1 || burnin < 0 || maxepoch < 0 || L < 1 || !(signal_var > 0)) {
    set_error("bad GPT_GMC arguments"); return GPT_ERR_BAD_DIMS;
  }
  if (!rank_supported((int)r) || !gmc_supported((int)n, (int)r)) {
    set_error("GPT_GMC: rank not instantiated or n*r too large for one workgroup's LDS");
    return GPT_ERR_BAD_DIMS;
  }
  std::vector<int32_t> I0;
  if (!zero_based_I(I, Q, D, r, I0)) return GPT_ERR_BAD_DIMS;
  const size_t nm = (size_t)n * r * D;
  std::vector<double> w0((size_t)Q), U0(nm);
  host_init_state((int)n, (int)r, (int)D, (int)Q, seed, true, 1.0, w0.data(), U0.data());
  if (w_init) std::memcpy(w0.data(), w_init, 8 * (size_t)Q);
  if (U_init) std::memcpy(U0.data(), U_init, 8 * nm);
  DevMem dphi, dy, dI, dw, dU, dst;
  GPT_HIPCHK(dphi.upload(phi, (size_t)n * D * N));
  GPT_HIPCHK(dy.upload(y, (size_t)N));
  GPT_HIPCHK(dI.upload(I0.data(), I0.size()));
  GPT_HIPCHK(dw.upload(w0.data(), w0.size()));
  GPT_HIPCHK(dU.upload(U0.data(), U0.size()));
  GPT_HIPCHK(dst.alloc<int32_t>(1));
  GPT_HIPCHK(dst.zero());
  std::memset(w_store, 0, 8 * (size_t)Q * maxepoch);
  std::memset(U_store, 0, 8 * nm * maxepoch);
  hipError_t e = gmc_run(dphi.as<double>(), dy.as<double>(), dI.as<int32_t>(), (int)n, (int)D, N,
                         (int)r, (int)Q, signal_var, epsw, epsU, (int)burnin, (int)maxepoch, (int)L,
                         seed, dw.as<double>(), dU.as<double>(), w_store, U_store, accept_prob,
                         dst.as<int32_t>(), nullptr);
  if (e != hipSuccess) return hip_fail(e, "GPT_GMC");
  int32_t bad = 0;
  GPT_HIPCHK(dst.download(&bad, 1));
  if (bad) {                         // GPT_SGLD.jl:757: zeros and NaN acceptance probabilities
    std::memset(w_store, 0, 8 * (size_t)Q * maxepoch);
    std::memset(U_store, 0, 8 * nm * maxepoch);
    for (int64_t z = 0; z < burnin + maxepoch; ++z) accept_prob[z] = std::nan("");
    set_error("Get NaN when moving along Geodesic. Try smaller epsU");
    return GPT_ERR_NAN_GEODESIC;
  }
  return GPT_OK;
}
