// Full-theta regression from host arrays: sibling GPNT_SGLD chains (gpnt.hip) from phi or from X,
// and the evaluation of stored samples: test RMSE per sample and of the prediction averaged over
// a window of samples (PowerPlantNoTensorExperiment.jl:42-63).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "eval_frame.h"

using namespace gpt;

// gpt_gpnt_last_route / gpt_gpnt_last_timing of this thread
static thread_local int32_t g_gpnt_route[3] = {0, 0, 0};
static thread_local double g_gpnt_ms[2] = {0.0, 0.0};

extern "C" int gpt_gpnt_last_route(int32_t* out, int32_t len) {
  if (!out || len < 0) { set_error("gpt_gpnt_last_route: bad output"); return GPT_ERR_BAD_DIMS; }
  for (int32_t x = 0; x < len; ++x) out[x] = x < 3 ? g_gpnt_route[x] : 0;
  return GPT_OK;
}

extern "C" int gpt_gpnt_last_timing(double* ms, int32_t len) {
  if (!ms || len < 0) { set_error("gpt_gpnt_last_timing: bad output"); return GPT_ERR_BAD_DIMS; }
  for (int32_t x = 0; x < len; ++x) ms[x] = x < 2 ? g_gpnt_ms[x] : 0.0;
  return GPT_OK;
}

// GPTSGLD_GPNT_ROWS=<g> (read on every call): at most g staged rows per group, 0 = no staging;
// -1 when unset or not a number
static int gpnt_rows_cap() {
  const char* ev = std::getenv("GPTSGLD_GPNT_ROWS");
  if (!ev || !*ev) return -1;
  char* end = nullptr;
  const long v = std::strtol(ev, &end, 10);
  if (end == ev || v < 0) return -1;
  return (int)std::min<long>(v, 1 << 30);
}

struct GpntRun : ThetaRun {
  GpntLayout L;
};

static bool gpnt_run_info(const void* data, const double* y, int64_t n, int64_t N, int64_t m,
                          const double* signal_var, const double* sigma_theta,
                          const double* eps_theta, int64_t burnin, int64_t maxepoch,
                          const uint64_t* seeds, int32_t nchains, int64_t store_every,
                          const double* theta_store, const int32_t* status, GpntRun* R) {
  if (!data || !y || !signal_var || !sigma_theta || !eps_theta || !seeds || !theta_store || !status) {
    set_error("gpt_gpnt_sgld_chains: null argument"); return false;
  }
  if (!theta_chain_dims_ok(n, N, m, burnin, maxepoch, nchains, store_every) ||
      m > (1LL << 31) - 1) {
    set_error("bad GPNT_SGLD_chains dimensions"); return false;
  }
  R->L = gpnt_layout((int)n, (int)N, (int)m, gpnt_rows_cap());
  if (R->L.base > (size_t)kMaxLds) {
    set_error("GPNT_SGLD_chains: theta (n) and the batch's bookkeeping exceed 160 KiB of LDS");
    return false;
  }
  static_cast<ThetaRun&>(*R) = ThetaRun(N, m, burnin, maxepoch, store_every);
  return true;
}

// The chains on device features dphi (n, N); y and every other array are the host's.
static int gpnt_chains_core(const double* dphi, const double* y, int64_t n, int64_t N, int64_t m,
                            const double* signal_var, const double* sigma_theta,
                            const double* eps_theta, double decay_rate, const uint64_t* seeds,
                            int32_t nchains, int64_t store_every, const GpntRun& R,
                            double* theta_store, int32_t* status) {
  ThetaChainSet S;
  const int rc = S.init(seeds, eps_theta, nchains, n, 1, N, R, sigma_theta, 1);
  if (rc != GPT_OK) return rc;
  std::vector<GpntChain> ch(nchains);
  for (int k = 0; k < nchains; ++k) ch[k] = GpntChain{S.chain(k), signal_var[k], sigma_theta[k]};
  DevMem dy, dch;
  GPT_HIPCHK(dy.upload(y, (size_t)N));
  GPT_HIPCHK(dch.upload(ch.data(), ch.size()));
  g_gpnt_route[0] = R.L.rows;
  g_gpnt_route[1] = R.L.groups;
  g_gpnt_route[2] = (int32_t)R.L.bytes;
  return S.run(R, &g_gpnt_ms[0], "gpnt_chain kernel", [&](long long t0, int nsteps) {
    return launch_gpnt_chain(dphi, dy.as<double>(), dch.as<GpntChain>(), nchains, (int)n, (int)N,
                             (int)m, (int)R.nb, R.total, decay_rate, (int)store_every, t0, nsteps,
                             R.L, nullptr);
  }, theta_store, status);
}

extern "C" int gpt_gpnt_sgld_chains(const double* phi, const double* y, int64_t n, int64_t N,
                                    int64_t m, const double* signal_var, const double* sigma_theta,
                                    const double* eps_theta, double decay_rate, int64_t burnin,
                                    int64_t maxepoch, const uint64_t* seeds, int32_t nchains,
                                    int64_t store_every, double* theta_store, int32_t* status) {
  GpntRun R;
  if (!gpnt_run_info(phi, y, n, N, m, signal_var, sigma_theta, eps_theta, burnin, maxepoch, seeds,
                     nchains, store_every, theta_store, status, &R))
    return GPT_ERR_BAD_DIMS;
  for (int k = 0; k < nchains; ++k) status[k] = 0;
  if (R.total == 0) return GPT_OK;
  DevMem dphi;
  GPT_HIPCHK(dphi.upload(phi, (size_t)n * N));
  return gpnt_chains_core(dphi.as<double>(), y, n, N, m, signal_var, sigma_theta, eps_theta,
                          decay_rate, seeds, nchains, store_every, R, theta_store, status);
}

extern "C" int gpt_gpnt_sgld_chains_x(const double* X, const double* y, int64_t N, int64_t D,
                                      const double* length_scale, int64_t ls_len, double sigma_rbf,
                                      const double* Z, const double* b, int64_t n, int64_t m,
                                      const double* signal_var, const double* sigma_theta,
                                      const double* eps_theta, double decay_rate, int64_t burnin,
                                      int64_t maxepoch, const uint64_t* seeds, int32_t nchains,
                                      int64_t store_every, double* theta_store, int32_t* status) {
  GpntRun R;
  if (!gpnt_run_info(X, y, n, N, m, signal_var, sigma_theta, eps_theta, burnin, maxepoch, seeds,
                     nchains, store_every, theta_store, status, &R) ||
      !valid_feature_args(length_scale, ls_len, D, Z, b))
    return GPT_ERR_BAD_DIMS;
  for (int k = 0; k < nchains; ++k) status[k] = 0;
  if (R.total == 0) return GPT_OK;
  DevMem dphi;
  GPT_TRY(device_features(false, X, N, D, length_scale, ls_len, sigma_rbf, 1.0, Z, b, n, dphi));
  return gpnt_chains_core(dphi.as<double>(), y, n, N, m, signal_var, sigma_theta, eps_theta,
                          decay_rate, seeds, nchains, store_every, R, theta_store, status);
}

// ---------------------------------------------------------------------------------- evaluation
static bool valid_gpnt_pred(const void* theta, const void* data, const void* ytest, int64_t n,
                            int64_t Ntest, int64_t T, int64_t avg_first, int64_t avg_last,
                            const void* sample_rmse, const void* mean, const void* rmse) {
  if (!theta || !data || !ytest || !sample_rmse || !mean || !rmse) {
    set_error("gpt_gpnt_pred: null argument"); return false;
  }
  if (n < 1 || Ntest < 1 || T < 1 || n > (1 << 24) || T > (1 << 22) || Ntest > (1LL << 40)) {
    set_error("gpt_gpnt_pred: bad dimensions"); return false;
  }
  return window_ok("gpt_gpnt_pred", "avg_", avg_first, avg_last, T);
}

// scores (Ntest, T) = phitestᵀ·theta on device features, then the window's figures and its mean.
static int gpnt_pred_core(const double* theta, const double* dphi, const double* ytest, int64_t n,
                          int64_t Ntest, int64_t T, int64_t avg_first, int64_t avg_last,
                          double scale, double* sample_rmse_out, double* mean_out,
                          double* rmse_out, double* scores_out) {
  DevMem dy;
  ThetaScores sc{n, Ntest, T};
  WindowRmse ev{Ntest, T, avg_first, avg_last - avg_first};
  GPT_TRY(sc.stage(theta));
  GPT_HIPCHK(dy.upload(ytest, (size_t)Ntest));
  GPT_TRY(ev.stage(true));
  {
    EventTimer tm(&g_gpnt_ms[1], nullptr);
    GPT_TRY(sc.launch(dphi));
    GPT_TRY(ev.launch(sc.s.as<double>(), dy.as<double>()));
    tm.stop();
    GPT_HIPCHK(hipStreamSynchronize(nullptr));
  }
  GPT_TRY(ev.fetch(scale, sample_rmse_out, rmse_out, mean_out));
  if (scores_out) GPT_HIPCHK(sc.s.download(scores_out, (size_t)Ntest * T));
  return GPT_OK;
}

extern "C" int gpt_gpnt_pred(const double* theta, const double* phitest, const double* ytest,
                             int64_t n, int64_t Ntest, int64_t T, int64_t avg_first,
                             int64_t avg_last, double scale, double* sample_rmse_out,
                             double* mean_out, double* rmse_out, double* scores_out) {
  if (!valid_gpnt_pred(theta, phitest, ytest, n, Ntest, T, avg_first, avg_last, sample_rmse_out,
                       mean_out, rmse_out))
    return GPT_ERR_BAD_DIMS;
  DevMem dphi;
  GPT_HIPCHK(dphi.upload(phitest, (size_t)n * Ntest));
  return gpnt_pred_core(theta, dphi.as<double>(), ytest, n, Ntest, T, avg_first, avg_last, scale,
                        sample_rmse_out, mean_out, rmse_out, scores_out);
}

extern "C" int gpt_gpnt_pred_x(const double* theta, const double* Xtest, const double* ytest,
                               int64_t Ntest, int64_t D, const double* length_scale,
                               int64_t ls_len, double sigma_rbf, const double* Z, const double* b,
                               int64_t n, int64_t T, int64_t avg_first, int64_t avg_last,
                               double scale, double* sample_rmse_out, double* mean_out,
                               double* rmse_out, double* scores_out) {
  if (!valid_gpnt_pred(theta, Xtest, ytest, n, Ntest, T, avg_first, avg_last, sample_rmse_out,
                       mean_out, rmse_out) ||
      !valid_feature_args(length_scale, ls_len, D, Z, b))
    return GPT_ERR_BAD_DIMS;
  DevMem dphi;
  GPT_TRY(device_features(false, Xtest, Ntest, D, length_scale, ls_len, sigma_rbf, 1.0, Z, b, n, dphi));
  return gpnt_pred_core(theta, dphi.as<double>(), ytest, n, Ntest, T, avg_first, avg_last, scale,
                        sample_rmse_out, mean_out, rmse_out, scores_out);
}
