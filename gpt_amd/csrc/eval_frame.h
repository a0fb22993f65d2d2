// Host frame of the entries that turn stored samples into predictions and judge them (api_pred,
// api_gpnt, api_cls, api_predictive): the feature inputs formed from X, the tensor samples and the
// full-theta scores on the device, the window check and the RMSE figures.  Every launch goes to the
// null stream.  No device code.
#pragma once
#include <cmath>
#include "host_util.h"

namespace gpt {

// ---- feature inputs from X --------------------------------------------------------------------
inline bool ls_len_ok(int64_t ls_len, int64_t D) {
  if (ls_len == 1 || ls_len == D) return true;
  set_error("dimensions of X and length_scale do not match");
  return false;
}
// The feature checks of the full-theta entries that take X.
inline bool valid_feature_args(const double* ls, int64_t ls_len, int64_t D, const double* Z,
                               const double* b) {
  if (!ls || !Z || !b || D < 1 || D > (1 << 20)) { set_error("bad feature arguments"); return false; }
  return ls_len_ok(ls_len, D);
}
// The constant of feature_kernel (tensor model) and of feature_notensor_kernel.
inline double tensor_feature_c(double sigma_rbf, double phi_scale, int64_t D, int64_t n) {
  return phi_scale * std::pow(sigma_rbf, 1.0 / (double)D) * std::sqrt(2.0 / (double)n);
}
inline double notensor_feature_c(double sigma_rbf, int64_t n) {
  return std::sqrt(2.0 / (double)n) * sigma_rbf;
}
// X (rows, D), the length scale expanded to one entry per dimension, Z (n, D) and b, which has
// n·D entries in the tensor model and n without it.
struct FeatureInputs {
  DevMem X, ls, Z, b;
  int upload(const double* X_, int64_t rows, int64_t D, const double* ls_, int64_t ls_len,
             const double* Z_, const double* b_, int64_t n, bool tensor) {
    std::vector<double> lsv(D);
    for (int64_t k = 0; k < D; ++k) lsv[k] = ls_[ls_len == 1 ? 0 : k];
    GPT_HIPCHK(X.upload(X_, (size_t)rows * D));
    GPT_HIPCHK(ls.upload(lsv.data(), lsv.size()));
    GPT_HIPCHK(Z.upload(Z_, (size_t)n * D));
    GPT_HIPCHK(b.upload(b_, tensor ? (size_t)n * D : (size_t)n));
    return GPT_OK;
  }
};
// api_pred.hip: dphi = feature (n, D, rows) or featureNotensor (n, rows) of X, formed on the device
int device_features(bool tensor, const double* X, int64_t rows, int64_t D, const double* ls,
                    int64_t ls_len, double sigma_rbf, double phi_scale, const double* Z,
                    const double* b, int64_t n, DevMem& dphi);

// ---- tensor samples ---------------------------------------------------------------------------
// w (Q, S), U (n, r, D, S) and the 0-based table of I (Q, D, 1-based), which is checked first.
struct TensorSamples {
  DevMem w, U, I;
  int upload(const double* w_, const double* U_, const int32_t* I_, int64_t n, int64_t D,
             int64_t r, int64_t Q, int64_t S) {
    std::vector<int32_t> I0;
    if (!zero_based_I(I_, Q, D, r, I0)) return GPT_ERR_BAD_DIMS;
    GPT_HIPCHK(w.upload(w_, (size_t)Q * S));
    GPT_HIPCHK(U.upload(U_, (size_t)n * r * D * S));
    GPT_HIPCHK(I.upload(I0.data(), I0.size()));
    return GPT_OK;
  }
};
// api_pred.hip: fhat (Ntest, S) of S tensor samples from host arrays into df, as gpt_pred_mean
// (gpt_pred_dev timed into *ms when given) and gpt_pred_mean_x (its checks and routes) form them
int pred_store_fhat(const double* w, const double* U, const int32_t* I, const double* phitest,
                    int64_t n, int64_t D, int64_t Ntest, int64_t r, int64_t Q, int64_t S, DevMem& df,
                    double* ms = nullptr);
int pred_store_fhat_x(const double* w_store, const double* U_store, const int32_t* I,
                      const double* Xtest, const double* ytest, int64_t Ntest, int64_t D,
                      const double* length_scale, int64_t ls_len, double sigma_rbf, double phi_scale,
                      const double* Z, const double* b, int64_t n, int64_t r, int64_t Q, int64_t S,
                      DevMem& df);

// ---- full-theta scores ------------------------------------------------------------------------
// s (Ntest, cols) = phitestᵀ·theta of theta (n, cols) on device features (n, Ntest).  The upload
// and the launch are two steps so that a caller's timer spans the kernel alone.
struct ThetaScores {
  int64_t n, Ntest, cols;
  DevMem th, s;
  int stage(const double* theta) {
    GPT_HIPCHK(th.upload(theta, (size_t)n * cols));
    GPT_HIPCHK(s.alloc<double>((size_t)Ntest * cols));
    return GPT_OK;
  }
  int launch(const double* dphi) const {
    const hipError_t e =
        launch_nt_scores(dphi, th.as<double>(), (int)n, Ntest, cols, s.as<double>(), nullptr);
    return e == hipSuccess ? GPT_OK : hip_fail(e, "nt_scores kernel");
  }
};

// ---- the window and the RMSE figures ----------------------------------------------------------
// The half-open window of samples; the entry `who` names its bounds <pre>first and <pre>last.
inline bool window_ok(const char* who, const char* pre, int64_t first, int64_t last, int64_t T) {
  if (first >= 0 && last <= T && first < last) return true;
  set_error(std::string(who) + ": the window must satisfy 0 <= " + pre + "first < " + pre +
            "last <= T");
  return false;
}
inline double rmse_of(double scale, double sse, int64_t Ntest) {
  return scale * std::sqrt(sse / (double)Ntest);
}
// Device predictions F (Ntest, T) against device y: mean_sse_kernel on all T columns for the
// per-sample figures, then on the window's for its mean's; the mean itself (Ntest) is kept when
// asked for.  launch() drains nothing; fetch() copies on the null stream, so after the kernels.
struct WindowRmse {
  int64_t Ntest, T, first, S;                  // S = last - first samples in the window
  DevMem sse, win, mean;
  int stage(bool want_mean) {
    if (want_mean) GPT_HIPCHK(mean.alloc<double>((size_t)Ntest));
    GPT_HIPCHK(sse.alloc<double>((size_t)T + 1));
    GPT_HIPCHK(win.alloc<double>((size_t)S + 1));
    return GPT_OK;
  }
  int launch(const double* F, const double* y) const {
    hipError_t e = launch_mean_rmse(F, y, Ntest, (int)T, nullptr, sse.as<double>(), nullptr);
    if (e == hipSuccess)
      e = launch_mean_rmse(F + (size_t)first * Ntest, y, Ntest, (int)S, mean.as<double>(),
                           win.as<double>(), nullptr);
    return e == hipSuccess ? GPT_OK : hip_fail(e, "mean/sse kernel");
  }
  // each output may be null; mean_out needs want_mean
  int fetch(double scale, double* sample_rmse, double* rmse, double* mean_out) const {
    std::vector<double> h((size_t)T + 1);
    double wsse = 0.0;
    GPT_HIPCHK(sse.download(h.data(), h.size()));
    GPT_HIPCHK(win.download(&wsse, 1));
    if (mean_out) GPT_HIPCHK(mean.download(mean_out, (size_t)Ntest));
    if (sample_rmse)
      for (int64_t t = 0; t < T; ++t) sample_rmse[t] = rmse_of(scale, h[1 + t], Ntest);
    if (rmse) *rmse = rmse_of(scale, wsse, Ntest);
    return GPT_OK;
  }
};
// The one-launch form over all S samples of device fhat (Ntest, S) against the host's ytest: the
// mean prediction, its RMSE and the per-sample RMSE, each optional (gpt_pred_mean, gpt_pred_mean_x).
inline int all_samples_rmse(const DevMem& df, const double* ytest, int64_t Ntest, int64_t S,
                            double scale, double* mean_out, double* rmse_out,
                            double* sample_rmse_out) {
  DevMem dy, dmean, dsse;
  GPT_HIPCHK(dy.upload(ytest, (size_t)Ntest));
  GPT_HIPCHK(dmean.alloc<double>((size_t)Ntest));
  GPT_HIPCHK(dsse.alloc<double>((size_t)(S + 1)));
  const hipError_t e = launch_mean_rmse(df.as<double>(), dy.as<double>(), Ntest, (int)S,
                                        dmean.as<double>(), dsse.as<double>(), nullptr);
  if (e != hipSuccess) return hip_fail(e, "mean/sse kernel");
  std::vector<double> sse(sample_rmse_out ? (size_t)S + 1 : 1);
  GPT_HIPCHK(dsse.download(sse.data(), sse.size()));
  if (mean_out) GPT_HIPCHK(dmean.download(mean_out, (size_t)Ntest));
  if (rmse_out) *rmse_out = rmse_of(scale, sse[0], Ntest);
  for (size_t z = 1; z < sse.size(); ++z) sample_rmse_out[z - 1] = rmse_of(scale, sse[z], Ntest);
  return GPT_OK;
}

}  // namespace gpt
