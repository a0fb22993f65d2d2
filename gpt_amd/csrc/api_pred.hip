// Features and predictions from host arrays (gpt_feature*, gpt_pred*), the device-pointer
// prediction entries and the prediction route queries.
#include <cstdlib>
#include <cstring>
#include <optional>

#include "eval_frame.h"

using namespace gpt;

// dphi = feature (n, D, rows) or featureNotensor (n, rows) of X formed on the device, the doubles
// of gpt_feature*.  The inputs are freed on return, after the stream has drained.
int gpt::device_features(bool tensor, const double* X, int64_t rows, int64_t D, const double* ls,
                         int64_t ls_len, double sigma_rbf, double phi_scale, const double* Z,
                         const double* b, int64_t n, DevMem& dphi) {
  FeatureInputs in;
  GPT_TRY(in.upload(X, rows, D, ls, ls_len, Z, b, n, tensor));
  GPT_HIPCHK(dphi.alloc<double>((size_t)n * rows * (tensor ? D : 1)));
  const double c = tensor ? tensor_feature_c(sigma_rbf, phi_scale, D, n)
                          : notensor_feature_c(sigma_rbf, n);
  const hipError_t e = (tensor ? launch_feature : launch_feature_notensor)(
      in.X.as<double>(), rows, (int)D, in.ls.as<double>(), c, in.Z.as<double>(), in.b.as<double>(),
      (int)n, dphi.as<double>(), nullptr);
  if (e != hipSuccess) return hip_fail(e, "feature kernel");
  GPT_HIPCHK(hipStreamSynchronize(nullptr));
  return GPT_OK;
}

static int feature_common(bool tensor, const double* X, int64_t N, int64_t D, const double* ls,
                          int64_t ls_len, double sigma_rbf, double phi_scale, const double* Z,
                          const double* b, int64_t n, double* phi_out) {
  if (!X || !ls || !Z || !b || !phi_out || N < 1 || D < 1 || n < 1) {
    set_error("bad feature arguments"); return GPT_ERR_BAD_DIMS;
  }
  if (!ls_len_ok(ls_len, D)) return GPT_ERR_BAD_DIMS;
  DevMem dphi;
  GPT_TRY(device_features(tensor, X, N, D, ls, ls_len, sigma_rbf, phi_scale, Z, b, n, dphi));
  GPT_HIPCHK(dphi.download(phi_out, dphi.bytes / sizeof(double)));
  return GPT_OK;
}

extern "C" int gpt_feature_dev(const double* X_dev, int64_t N, int64_t D, const double* ls_dev,
                               int64_t ls_len, double sigma_rbf, double phi_scale,
                               const double* Z_dev, const double* b_dev, int64_t n, double* phi_dev,
                               void* hip_stream) {
  if (!X_dev || !ls_dev || !Z_dev || !b_dev || !phi_dev || N < 1 || D < 1 || n < 1 || ls_len != D) {
    set_error("bad gpt_feature_dev arguments (ls_len must equal D)"); return GPT_ERR_BAD_DIMS;
  }
  const double c = tensor_feature_c(sigma_rbf, phi_scale, D, n);
  const hipError_t e = launch_feature(X_dev, N, (int)D, ls_dev, c, Z_dev, b_dev, (int)n, phi_dev,
                                      (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_fail(e, "feature kernel");
  return GPT_OK;
}

extern "C" int gpt_feature(const double* X, int64_t N, int64_t D, const double* length_scale,
                           int64_t ls_len, double sigma_rbf, double phi_scale, const double* Z,
                           const double* b, int64_t n, double* phi_out) {
  return feature_common(true, X, N, D, length_scale, ls_len, sigma_rbf, phi_scale, Z, b, n, phi_out);
}

extern "C" int gpt_feature_notensor(const double* X, int64_t N, int64_t D, const double* length_scale,
                                    int64_t ls_len, double sigma_rbf, const double* Z,
                                    const double* b, int64_t n, double* phi_out) {
  return feature_common(false, X, N, D, length_scale, ls_len, sigma_rbf, 1.0, Z, b, n, phi_out);
}

bool gpt::valid_pred(int64_t n, int64_t D, int64_t Ntest, int64_t r, int64_t Q) {
  if (n < 1 || D < 1 || Ntest < 0 || r < 1 || Q < 1) { set_error("bad pred dims"); return false; }
  if (D > kDMax) { set_error("D > 16 unsupported"); return false; }
  if (!rank_supported((int)r)) { set_error("rank not instantiated"); return false; }
  if (pred_lds_bytes((int)n, (int)D, (int)r, (int)Q) > kMaxLds) { set_error("pred LDS too large"); return false; }
  return true;
}

extern "C" int gpt_pred_dev(const double* w_dev, const double* U_dev, const int32_t* I0_dev,
                            const double* phitest_dev, int64_t n, int64_t D, int64_t Ntest,
                            int64_t r, int64_t Q, int64_t S, double* fhat_dev, void* hip_stream) {
  if (!valid_pred(n, D, Ntest, r, Q)) return GPT_ERR_BAD_DIMS;
  hipError_t e = launch_pred(w_dev, U_dev, I0_dev, phitest_dev, (int)n, (int)D, Ntest, (int)r,
                             (int)Q, (int)S, fhat_dev, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_fail(e, "pred kernel");
  return GPT_OK;
}

extern "C" int gpt_pred_trim_pool(void) {
  GPT_HIPCHK(pred_trim_pools());
  return GPT_OK;
}

extern "C" int gpt_pred_dev_timed(const double* w_dev, const double* U_dev, const int32_t* I0_dev,
                                  const double* phitest_dev, int64_t n, int64_t D, int64_t Ntest,
                                  int64_t r, int64_t Q, int64_t S, double* fhat_dev,
                                  void* hip_stream, double* ms_out) {
  if (!valid_pred(n, D, Ntest, r, Q)) return GPT_ERR_BAD_DIMS;
  if (!ms_out) { set_error("gpt_pred_dev_timed: ms_out is null"); return GPT_ERR_BAD_DIMS; }
  PredPhaseTiming tm;
  hipError_t e = launch_pred(w_dev, U_dev, I0_dev, phitest_dev, (int)n, (int)D, Ntest, (int)r,
                             (int)Q, (int)S, fhat_dev, (hipStream_t)hip_stream, &tm);
  if (e != hipSuccess) return hip_fail(e, "pred kernel");
  GPT_HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
  ms_out[0] = tm.gemm_ms;
  ms_out[1] = tm.vphase_ms;
  return GPT_OK;
}

// fhat (Ntest, S) of S stored samples into df, from host arrays (I 1-based): the prediction of
// gpt_pred_mean and the scores of gpt_pred_class; *ms, when given, times gpt_pred_dev alone.  The
// uploads are freed on return, after the stream has drained.
int gpt::pred_store_fhat(const double* w, const double* U, const int32_t* I, const double* phitest,
                         int64_t n, int64_t D, int64_t Ntest, int64_t r, int64_t Q, int64_t S,
                         DevMem& df, double* ms) {
  if (!valid_pred(n, D, Ntest, r, Q) || S < 1) return GPT_ERR_BAD_DIMS;
  TensorSamples ts;
  DevMem dphi;
  GPT_TRY(ts.upload(w, U, I, n, D, r, Q, S));
  GPT_HIPCHK(dphi.upload(phitest, (size_t)n * D * Ntest));
  GPT_HIPCHK(df.alloc<double>((size_t)Ntest * S));
  {
    std::optional<EventTimer> tm;
    if (ms) tm.emplace(ms, nullptr);
    GPT_TRY(gpt_pred_dev(ts.w.as<double>(), ts.U.as<double>(), ts.I.as<int32_t>(), dphi.as<double>(),
                         n, D, Ntest, r, Q, S, df.as<double>(), nullptr));
    if (tm) tm->stop();
  }
  GPT_HIPCHK(hipStreamSynchronize(nullptr));
  return GPT_OK;
}

extern "C" int gpt_pred(const double* w, const double* U, const int32_t* I, const double* phitest,
                        int64_t n, int64_t D, int64_t Ntest, int64_t r, int64_t Q, double* fhat_out) {
  DevMem df;
  GPT_TRY(pred_store_fhat(w, U, I, phitest, n, D, Ntest, r, Q, 1, df));
  if (fhat_out) GPT_HIPCHK(df.download(fhat_out, (size_t)Ntest));
  GPT_HIPCHK(hipStreamSynchronize(nullptr));   // every launch and copy of the call went to it
  return GPT_OK;
}

extern "C" int gpt_pred_mean(const double* w_store, const double* U_store, const int32_t* I,
                             const double* phitest, const double* ytest, int64_t n, int64_t D,
                             int64_t Ntest, int64_t r, int64_t Q, int64_t S, double scale,
                             double* mean_out, double* rmse_out) {
  if (!ytest) { set_error("ytest required"); return GPT_ERR_BAD_DIMS; }
  DevMem df;
  GPT_TRY(pred_store_fhat(w_store, U_store, I, phitest, n, D, Ntest, r, Q, S, df));
  GPT_TRY(all_samples_rmse(df, ytest, Ntest, S, scale, mean_out, rmse_out, nullptr));
  GPT_HIPCHK(hipStreamSynchronize(nullptr));   // as gpt_pred
  return GPT_OK;
}

// fhat (Ntest, S) of S stored samples into df with the test features formed on the device from
// Xtest: the prediction of gpt_pred_mean_x, its checks included.
int gpt::pred_store_fhat_x(const double* w_store, const double* U_store, const int32_t* I,
                           const double* Xtest, const double* ytest, int64_t Ntest, int64_t D,
                           const double* length_scale, int64_t ls_len, double sigma_rbf,
                           double phi_scale, const double* Z, const double* b, int64_t n, int64_t r,
                           int64_t Q, int64_t S, DevMem& df) {
  if (!w_store || !U_store || !I || !Xtest || !ytest || !length_scale || !Z || !b || S < 1) {
    set_error("bad pred_mean_x arguments"); return GPT_ERR_BAD_DIMS;
  }
  if (!ls_len_ok(ls_len, D) || !valid_pred(n, D, Ntest, r, Q)) return GPT_ERR_BAD_DIMS;
  if (pred_x_lds_bytes((int)n, (int)D, (int)r, (int)Q) > kMaxLds) {
    set_error("pred LDS too large"); return GPT_ERR_BAD_DIMS;
  }
  const double c = tensor_feature_c(sigma_rbf, phi_scale, D, n);
  TensorSamples ts;
  FeatureInputs in;
  GPT_TRY(ts.upload(w_store, U_store, I, n, D, r, Q, S));
  GPT_TRY(in.upload(Xtest, Ntest, D, length_scale, ls_len, Z, b, n, true));
  GPT_HIPCHK(df.alloc<double>((size_t)Ntest * S));
  // Default: the test features are formed once on the device (feature_kernel, the same doubles
  // as gpt_feature) and every sample is predicted by the stacked-sample MFMA path, which reads
  // them through L2 per group of samples.  GPTSGLD_PRED=direct: pred_x_kernel, which forms the
  // features inside every sample's prediction tile (no phitest array).
  const char* pev = std::getenv("GPTSGLD_PRED");
  hipError_t e;
  DevMem dphi;
  if (pev && std::strcmp(pev, "direct") == 0) {
    e = launch_pred_x(ts.w.as<double>(), ts.U.as<double>(), ts.I.as<int32_t>(), in.X.as<double>(),
                      in.ls.as<double>(), in.Z.as<double>(), in.b.as<double>(), c, (int)n, (int)D,
                      Ntest, (int)r, (int)Q, (int)S, df.as<double>(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "pred_x kernel");
  } else {
    GPT_HIPCHK(dphi.alloc<double>((size_t)n * D * Ntest));
    e = launch_feature(in.X.as<double>(), Ntest, (int)D, in.ls.as<double>(), c, in.Z.as<double>(),
                       in.b.as<double>(), (int)n, dphi.as<double>(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "feature kernel");
    e = launch_pred(ts.w.as<double>(), ts.U.as<double>(), ts.I.as<int32_t>(), dphi.as<double>(), (int)n,
                    (int)D, Ntest, (int)r, (int)Q, (int)S, df.as<double>(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "pred kernels");
  }
  GPT_HIPCHK(hipStreamSynchronize(nullptr));
  return GPT_OK;
}

extern "C" int gpt_pred_mean_x(const double* w_store, const double* U_store, const int32_t* I,
                               const double* Xtest, const double* ytest, int64_t Ntest, int64_t D,
                               const double* length_scale, int64_t ls_len, double sigma_rbf,
                               double phi_scale, const double* Z, const double* b, int64_t n,
                               int64_t r, int64_t Q, int64_t S, double scale, double* mean_out,
                               double* rmse_out, double* sample_rmse_out) {
  DevMem df;
  GPT_TRY(pred_store_fhat_x(w_store, U_store, I, Xtest, ytest, Ntest, D, length_scale, ls_len,
                            sigma_rbf, phi_scale, Z, b, n, r, Q, S, df));
  return all_samples_rmse(df, ytest, Ntest, S, scale, mean_out, rmse_out, sample_rmse_out);
}

extern "C" int gpt_pred_last_vphase(int32_t* kind) {
  if (!kind) { set_error("gpt_pred_last_vphase: null output"); return GPT_ERR_BAD_DIMS; }
  *kind = pred_last_vphase();
  return GPT_OK;
}

extern "C" int gpt_pred_last_route(int32_t* out, int32_t len) {
  if (!out || len < 0) { set_error("gpt_pred_last_route: bad output"); return GPT_ERR_BAD_DIMS; }
  pred_last_route(out, (int)len);
  for (int32_t x = kPredRouteLen; x < len; ++x) out[x] = 0;
  return GPT_OK;
}
