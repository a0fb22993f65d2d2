// Chain diagnostics of a store (diag.hip) from host arrays or where the store lies on the device.
#include <cmath>
#include <vector>

#include "host_util.h"

using namespace gpt;

// gpt_diag_last_timing of this thread
static thread_local double g_dg_ms = 0.0;

extern "C" int gpt_diag_last_timing(double* ms) {
  if (!ms) { set_error("gpt_diag_last_timing: null output"); return GPT_ERR_BAD_DIMS; }
  *ms = g_dg_ms;
  return GPT_OK;
}

extern "C" int gpt_diag_tiling(int32_t* out, int32_t len) {
  if (!out || len < 3) { set_error("gpt_diag_tiling: needs room for 3 values"); return GPT_ERR_BAD_DIMS; }
  out[0] = diag_time_chunk();
  out[1] = diag_lag_block();
  out[2] = diag_lag_group();
  for (int32_t k = 3; k < len; ++k) out[k] = 0;
  return GPT_OK;
}

constexpr int64_t kDiagMaxDoubles = 1LL << 31;       // one upload of the host entry: 16 GiB

struct DiagOut {
  double *mean, *sd, *rhat, *ess, *mcse, *tau;
  int32_t* truncated;
  double *chain_mean, *chain_var, *acf, *chain_acf;
};

static bool valid_diag(const void* store, int64_t P, int64_t T, int64_t M, int64_t first,
                       int64_t last, int64_t max_lag, const DiagOut& o) {
  if (!store || !o.mean || !o.sd || !o.rhat || !o.ess || !o.mcse || !o.tau || !o.truncated) {
    set_error("chain_diag: null argument"); return false;
  }
  if (P < 1) { set_error("chain_diag: P must be >= 1"); return false; }
  if (T < 4 || T > (1 << 22)) { set_error("chain_diag: T must be in 4..2^22"); return false; }
  if (M < 1 || M > 1024) { set_error("chain_diag: M must be in 1..1024"); return false; }
  if (max_lag < 1 || max_lag > 4096) { set_error("chain_diag: max_lag must be in 1..4096"); return false; }
  if (first < 0 || last > T || first >= last) {
    set_error("chain_diag: the window must satisfy 0 <= first < last <= T"); return false;
  }
  if (last - first < 4) { set_error("chain_diag: the window needs last - first >= 4"); return false; }
  if (P > (1LL << 40)) { set_error("chain_diag: P must be <= 2^40"); return false; }
  return true;
}

// The evaluator on the device store into device outputs; synchronises st (the workspace is freed
// on return).
static int diag_core(const double* store, int64_t P, int64_t M, int64_t first, int64_t last,
                     int64_t max_lag, int64_t cstride, const DiagOut& o, hipStream_t st) {
  const int S = (int)(last - first), K = (int)std::min<int64_t>(max_lag, S - 1);
  DevMem ws;
  GPT_HIPCHK(ws.alloc<double>(diag_ws_doubles(P, (int)M, K)));
  EventTimer tm(&g_dg_ms, st);
  const hipError_t e = launch_chain_diag(store + (size_t)first * P, P, cstride, S, (int)M, K,
                                         ws.as<double>(), o.mean, o.sd, o.rhat, o.ess, o.mcse, o.tau,
                                         o.truncated, o.chain_mean, o.chain_var, o.acf, o.chain_acf, st);
  if (e != hipSuccess) return hip_fail(e, "chain_diag kernels");
  tm.stop();
  GPT_HIPCHK(hipStreamSynchronize(st));
  return GPT_OK;
}

extern "C" int gpt_chain_diag_dev(const double* store_dev, int64_t P, int64_t T, int64_t M,
                                  int64_t chain_stride, int64_t first, int64_t last, int64_t max_lag,
                                  double* mean_dev, double* sd_dev, double* rhat_dev, double* ess_dev,
                                  double* mcse_dev, double* tau_dev, int32_t* truncated_dev,
                                  double* chain_mean_dev, double* chain_var_dev, double* acf_dev,
                                  double* chain_acf_dev, void* hip_stream) {
  const DiagOut o{mean_dev, sd_dev, rhat_dev, ess_dev, mcse_dev, tau_dev, truncated_dev,
                  chain_mean_dev, chain_var_dev, acf_dev, chain_acf_dev};
  if (!valid_diag(store_dev, P, T, M, first, last, max_lag, o)) return GPT_ERR_BAD_DIMS;
  if (chain_stride < P * T || chain_stride > (1LL << 44)) {
    set_error("chain_diag: chain_stride must be >= P*T"); return GPT_ERR_BAD_DIMS;
  }
  return diag_core(store_dev, P, M, first, last, max_lag, chain_stride, o, (hipStream_t)hip_stream);
}

extern "C" int gpt_chain_diag(const double* store, int64_t P, int64_t T, int64_t M, int64_t first,
                              int64_t last, int64_t max_lag, double* mean, double* sd, double* rhat,
                              double* ess, double* mcse, double* tau, int32_t* truncated,
                              double* chain_mean, double* chain_var, double* acf, double* chain_acf) {
  const DiagOut h{mean, sd, rhat, ess, mcse, tau, truncated, chain_mean, chain_var, acf, chain_acf};
  if (!valid_diag(store, P, T, M, first, last, max_lag, h)) return GPT_ERR_BAD_DIMS;
  if (P > kDiagMaxDoubles / T / M) {
    set_error("chain_diag: the store must hold at most 2^31 doubles (16 GiB)"); return GPT_ERR_BAD_DIMS;
  }
  const size_t K1 = (size_t)std::min<int64_t>(max_lag, last - first - 1) + 1;
  const size_t np = (size_t)P, nm = np * (size_t)M;
  DevMem dx, drow[6], dtr, dcm, dcv, dacf, dca;
  GPT_HIPCHK(dx.upload(store, np * (size_t)T * (size_t)M));
  for (auto& d : drow) GPT_HIPCHK(d.alloc<double>(np));
  GPT_HIPCHK(dtr.alloc<int32_t>(np));
  if (chain_mean) GPT_HIPCHK(dcm.alloc<double>(nm));
  if (chain_var) GPT_HIPCHK(dcv.alloc<double>(nm));
  if (acf) GPT_HIPCHK(dacf.alloc<double>(np * K1));
  if (chain_acf) GPT_HIPCHK(dca.alloc<double>(nm * K1));
  const DiagOut d{drow[0].as<double>(), drow[1].as<double>(), drow[2].as<double>(),
                  drow[3].as<double>(), drow[4].as<double>(), drow[5].as<double>(),
                  dtr.as<int32_t>(), dcm.as<double>(), dcv.as<double>(), dacf.as<double>(),
                  dca.as<double>()};
  GPT_TRY(diag_core(dx.as<double>(), P, M, first, last, max_lag, P * T, d, nullptr));
  double* const host[6] = {mean, sd, rhat, ess, mcse, tau};
  for (int k = 0; k < 6; ++k) GPT_HIPCHK(drow[k].download(host[k], np));
  GPT_HIPCHK(dtr.download(truncated, np));
  if (chain_mean) GPT_HIPCHK(dcm.download(chain_mean, nm));
  if (chain_var) GPT_HIPCHK(dcv.download(chain_var, nm));
  if (acf) GPT_HIPCHK(dacf.download(acf, np * K1));
  if (chain_acf) GPT_HIPCHK(dca.download(chain_acf, nm * K1));
  return GPT_OK;
}
