// Posterior predictive of the sampled regression models (predictive.hip) from device or host
// predictions, and behind the predictions of stored tensor and full-theta samples, whose fhat
// stays on the device between the prediction and its evaluation.
#include <cmath>

#include "eval_frame.h"

using namespace gpt;

// gpt_predictive_last_timing of this thread
static thread_local double g_pv_ms = 0.0;

extern "C" int gpt_predictive_last_timing(double* ms) {
  if (!ms) { set_error("gpt_predictive_last_timing: null output"); return GPT_ERR_BAD_DIMS; }
  *ms = g_pv_ms;
  return GPT_OK;
}

static bool valid_predictive(const void* F, const void* y, int64_t Ntest, int64_t T, int64_t first,
                             int64_t last, double noise_var, const void* sums, const void* covered) {
  if (!F || !y || !sums || !covered) { set_error("predictive: null argument"); return false; }
  if (Ntest < 1 || T < 1 || T > (1 << 22) || Ntest > (1LL << 38)) {
    set_error("predictive: bad dimensions"); return false;
  }
  if (!window_ok("predictive", "", first, last, T)) return false;
  if (!std::isfinite(noise_var) || !(noise_var > 0.0)) {
    set_error("predictive: noise_var must be finite and > 0"); return false;
  }
  return true;
}

// The evaluator on device F (Ntest, T) / y into device rows (each optional) and host sums.
// Synchronises st (the workspace is freed on return).
static int predictive_core(const double* F, const double* y, int64_t Ntest, int64_t first,
                           int64_t last, double noise_var, double* fmu, double* fs2, double* lp,
                           double* lpmix, double* sums_host, double* covered_host, hipStream_t st) {
  const size_t ntiles = predictive_tiles(Ntest);
  DevMem dpart, dcov, dfin;
  GPT_HIPCHK(dpart.alloc<double>(2 * ntiles));
  GPT_HIPCHK(dcov.alloc<int32_t>(ntiles));
  GPT_HIPCHK(dfin.alloc<double>(3));
  {
    EventTimer tm(&g_pv_ms, st);
    const hipError_t e = launch_predictive(F + (size_t)first * Ntest, y, Ntest, (int)(last - first),
                                           noise_var, fmu, fs2, lp, lpmix, dpart.as<double>(),
                                           dcov.as<int32_t>(), dfin.as<double>(),
                                           dfin.as<double>() + 2, st);
    if (e != hipSuccess) return hip_fail(e, "predictive kernel");
    tm.stop();
    GPT_HIPCHK(hipStreamSynchronize(st));
  }
  double fin[3];
  GPT_HIPCHK(dfin.download(fin, 3));
  sums_host[0] = fin[0];
  sums_host[1] = fin[1];
  *covered_host = fin[2];
  return GPT_OK;
}

extern "C" int gpt_predictive_dev(const double* F_dev, const double* y_dev, int64_t Ntest, int64_t T,
                                  int64_t first, int64_t last, double noise_var, double* fmu_dev,
                                  double* fs2_dev, double* lp_dev, double* lpmix_dev,
                                  double* sums_host, double* covered_host, void* hip_stream) {
  if (!valid_predictive(F_dev, y_dev, Ntest, T, first, last, noise_var, sums_host, covered_host))
    return GPT_ERR_BAD_DIMS;
  return predictive_core(F_dev, y_dev, Ntest, first, last, noise_var, fmu_dev, fs2_dev, lp_dev,
                         lpmix_dev, sums_host, covered_host, (hipStream_t)hip_stream);
}

// The host outputs of every host-array entry; the rows and the RMSE figures may be null.
struct PvHostOut {
  double *fmu, *fs2, *lp, *lpmix, *sums, *covered, *rmse, *sample_rmse;
};

// Device predictions dF (Ntest, T) against the host's ytest: the window's RMSE figures, as
// gpt_gpnt_pred's, when either is asked for, then the evaluator on the window.
static int predictive_to_host(const double* dF, const double* ytest, int64_t Ntest, int64_t T,
                              int64_t first, int64_t last, double scale, double noise_var,
                              const PvHostOut& o) {
  DevMem dy, drow[4];
  GPT_HIPCHK(dy.upload(ytest, (size_t)Ntest));
  if (o.rmse || o.sample_rmse) {
    WindowRmse ev{Ntest, T, first, last - first};
    GPT_TRY(ev.stage(false));
    GPT_TRY(ev.launch(dF, dy.as<double>()));
    GPT_TRY(ev.fetch(scale, o.sample_rmse, o.rmse, nullptr));
  }
  double* const host[4] = {o.fmu, o.fs2, o.lp, o.lpmix};
  for (int k = 0; k < 4; ++k)
    if (host[k]) GPT_HIPCHK(drow[k].alloc<double>((size_t)Ntest));
  GPT_TRY(predictive_core(dF, dy.as<double>(), Ntest, first, last, noise_var, drow[0].as<double>(),
                          drow[1].as<double>(), drow[2].as<double>(), drow[3].as<double>(), o.sums,
                          o.covered, nullptr));
  for (int k = 0; k < 4; ++k)
    if (host[k]) GPT_HIPCHK(drow[k].download(host[k], (size_t)Ntest));
  return GPT_OK;
}

extern "C" int gpt_predictive(const double* F, const double* y, int64_t Ntest, int64_t T,
                              int64_t first, int64_t last, double noise_var, double* fmu_out,
                              double* fs2_out, double* lp_out, double* lpmix_out, double* sums_out,
                              double* covered_out, double* rmse_out, double* sample_rmse_out) {
  const PvHostOut o{fmu_out, fs2_out, lp_out, lpmix_out, sums_out, covered_out, rmse_out,
                    sample_rmse_out};
  if (!valid_predictive(F, y, Ntest, T, first, last, noise_var, o.sums, o.covered))
    return GPT_ERR_BAD_DIMS;
  DevMem dF;
  GPT_HIPCHK(dF.upload(F, (size_t)Ntest * T));
  return predictive_to_host(dF.as<double>(), y, Ntest, T, first, last, 1.0, noise_var, o);
}

// The checks the sample routes add to their prediction's own: the RMSE outputs are required.
static bool valid_route(const void* store, const void* ytest, int64_t Ntest, int64_t T,
                        int64_t first, int64_t last, double noise_var, const PvHostOut& o) {
  if (!o.rmse || !o.sample_rmse) { set_error("predictive: null argument"); return false; }
  return valid_predictive(store, ytest, Ntest, T, first, last, noise_var, o.sums, o.covered);
}

extern "C" int gpt_pred_predictive(const double* w_store, const double* U_store, const int32_t* I,
                                   const double* phitest, const double* ytest, int64_t n, int64_t D,
                                   int64_t Ntest, int64_t r, int64_t Q, int64_t S, double scale,
                                   int64_t first, int64_t last, double noise_var, double* fmu_out,
                                   double* fs2_out, double* lp_out, double* lpmix_out,
                                   double* sums_out, double* covered_out, double* rmse_out,
                                   double* sample_rmse_out) {
  const PvHostOut o{fmu_out, fs2_out, lp_out, lpmix_out, sums_out, covered_out, rmse_out,
                    sample_rmse_out};
  if (!w_store || !U_store || !I || !phitest) {
    set_error("predictive: null argument"); return GPT_ERR_BAD_DIMS;
  }
  if (!valid_route(w_store, ytest, Ntest, S, first, last, noise_var, o)) return GPT_ERR_BAD_DIMS;
  DevMem df;
  GPT_TRY(pred_store_fhat(w_store, U_store, I, phitest, n, D, Ntest, r, Q, S, df));
  return predictive_to_host(df.as<double>(), ytest, Ntest, S, first, last, scale, noise_var, o);
}

extern "C" int gpt_pred_predictive_x(const double* w_store, const double* U_store, const int32_t* I,
                                     const double* Xtest, const double* ytest, int64_t Ntest,
                                     int64_t D, const double* length_scale, int64_t ls_len,
                                     double sigma_rbf, double phi_scale, const double* Z,
                                     const double* b, int64_t n, int64_t r, int64_t Q, int64_t S,
                                     double scale, int64_t first, int64_t last, double noise_var,
                                     double* fmu_out, double* fs2_out, double* lp_out,
                                     double* lpmix_out, double* sums_out, double* covered_out,
                                     double* rmse_out, double* sample_rmse_out) {
  const PvHostOut o{fmu_out, fs2_out, lp_out, lpmix_out, sums_out, covered_out, rmse_out,
                    sample_rmse_out};
  if (!valid_route(w_store, ytest, Ntest, S, first, last, noise_var, o)) return GPT_ERR_BAD_DIMS;
  DevMem df;
  GPT_TRY(pred_store_fhat_x(w_store, U_store, I, Xtest, ytest, Ntest, D, length_scale, ls_len,
                            sigma_rbf, phi_scale, Z, b, n, r, Q, S, df));
  return predictive_to_host(df.as<double>(), ytest, Ntest, S, first, last, scale, noise_var, o);
}

// scores (Ntest, T) = phitestᵀ·theta on device features, as gpt_gpnt_pred forms them, evaluated
// where they are.
static int gpnt_predictive_core(const double* theta, const double* dphi, const double* ytest,
                                int64_t n, int64_t Ntest, int64_t T, int64_t first, int64_t last,
                                double scale, double noise_var, const PvHostOut& o) {
  ThetaScores sc{n, Ntest, T};
  GPT_TRY(sc.stage(theta));
  GPT_TRY(sc.launch(dphi));
  return predictive_to_host(sc.s.as<double>(), ytest, Ntest, T, first, last, scale, noise_var, o);
}

static bool valid_gpnt_route(const void* theta, const void* data, const void* ytest, int64_t n,
                             int64_t Ntest, int64_t T, int64_t first, int64_t last,
                             double noise_var, const PvHostOut& o) {
  if (!data) { set_error("predictive: null argument"); return false; }
  if (n < 1 || n > (1 << 24)) { set_error("predictive: bad dimensions"); return false; }
  return valid_route(theta, ytest, Ntest, T, first, last, noise_var, o);
}

extern "C" int gpt_gpnt_predictive(const double* theta, const double* phitest, const double* ytest,
                                   int64_t n, int64_t Ntest, int64_t T, int64_t first, int64_t last,
                                   double scale, double noise_var, double* fmu_out, double* fs2_out,
                                   double* lp_out, double* lpmix_out, double* sums_out,
                                   double* covered_out, double* rmse_out, double* sample_rmse_out) {
  const PvHostOut o{fmu_out, fs2_out, lp_out, lpmix_out, sums_out, covered_out, rmse_out,
                    sample_rmse_out};
  if (!valid_gpnt_route(theta, phitest, ytest, n, Ntest, T, first, last, noise_var, o))
    return GPT_ERR_BAD_DIMS;
  DevMem dphi;
  GPT_HIPCHK(dphi.upload(phitest, (size_t)n * Ntest));
  return gpnt_predictive_core(theta, dphi.as<double>(), ytest, n, Ntest, T, first, last, scale,
                              noise_var, o);
}

extern "C" int gpt_gpnt_predictive_x(const double* theta, const double* Xtest, const double* ytest,
                                     int64_t Ntest, int64_t D, const double* length_scale,
                                     int64_t ls_len, double sigma_rbf, const double* Z,
                                     const double* b, int64_t n, int64_t T, int64_t first,
                                     int64_t last, double scale, double noise_var, double* fmu_out,
                                     double* fs2_out, double* lp_out, double* lpmix_out,
                                     double* sums_out, double* covered_out, double* rmse_out,
                                     double* sample_rmse_out) {
  const PvHostOut o{fmu_out, fs2_out, lp_out, lpmix_out, sums_out, covered_out, rmse_out,
                    sample_rmse_out};
  if (!valid_gpnt_route(theta, Xtest, ytest, n, Ntest, T, first, last, noise_var, o) ||
      !valid_feature_args(length_scale, ls_len, D, Z, b))
    return GPT_ERR_BAD_DIMS;
  DevMem dphi;
  GPT_TRY(device_features(false, Xtest, Ntest, D, length_scale, ls_len, sigma_rbf, 1.0, Z, b, n, dphi));
  return gpnt_predictive_core(theta, dphi.as<double>(), ytest, n, Ntest, T, first, last, scale,
                              noise_var, o);
}
