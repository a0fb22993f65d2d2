// The samplers that take host arrays: one session per call (gpt_sgld_regression and its variants,
// the sibling-chain entries) and GPNT_SGLD.
#include <cstring>
#include <memory>
#include <vector>

#include "host_util.h"

using namespace gpt;

using SessionGuard = std::unique_ptr<gpt_sgld_session, void (*)(gpt_sgld_session*)>;

// Shared driver of the host-pointer samplers: one chain, device copies of phi / y, the run, the
// stores back (zero-filled + GPT_ERR_NAN_GEODESIC on the geodesic bail-out, GPT_SGLD.jl:422-424).
static int host_sampler(const gpt_sgld_config* cfg, const double* phi, const double* y,
                        const int32_t* I, const double* w_init, const double* U_init,
                        double* w_store, double* U_store, double* diag, int extra_flags,
                        double rms_eps, double rms_alpha, double* U_final = nullptr) {
  if (!valid_cfg(cfg)) return GPT_ERR_BAD_DIMS;
  if (!phi || !y || !I) { set_error("null input"); return GPT_ERR_BAD_DIMS; }
  DevMem dphi, dy;
  GPT_HIPCHK(dphi.upload(phi, (size_t)cfg->n * cfg->D * cfg->N));
  GPT_HIPCHK(dy.upload(y, (size_t)cfg->N));
  const double* pp = dphi.as<double>();
  const double* yy = dy.as<double>();
  gpt_sgld_session* s = nullptr;
  const int flags = ((w_store || U_store) ? kFlagStore : 0) | (diag ? kFlagDiag : 0) | extra_flags;
  GPT_TRY(gpt_sgld_session_create(cfg, 1, &cfg->seed, &pp, &yy, I, flags, nullptr, &s));
  SessionGuard guard(s, gpt_sgld_session_destroy);
  if (rms_eps > 0) GPT_TRY(gpt_sgld_session_set_rmsprop(s, rms_eps, rms_alpha));
  if (w_init || U_init) GPT_TRY(session_set_state(s, 0, w_init, U_init));
  GPT_TRY(gpt_sgld_session_run(s, session_run_info(s).total_steps));
  int32_t st = 0;
  GPT_TRY(gpt_sgld_session_fetch(s, 0, w_store, U_store, diag, &st));
  if (st) {
    set_error("Get NaN when moving along Geodesic. Try smaller epsU");
    return GPT_ERR_NAN_GEODESIC;
  }
  if (U_final)
    GPT_HIPCHK(hipMemcpy(U_final, session_run_info(s).U0, 8 * (size_t)cfg->n * cfg->r * cfg->D,
                         hipMemcpyDeviceToHost));
  return GPT_OK;
}

extern "C" int gpt_sgld_regression(const gpt_sgld_config* cfg, const double* phi, const double* y,
                                   const int32_t* I, const double* w_init, const double* U_init,
                                   double* w_store, double* U_store, double* diag) {
  return host_sampler(cfg, phi, y, I, w_init, U_init, w_store, U_store, diag, 0, 0.0, 0.0);
}

// The tail of the sibling-chain entries: per-chain hyper-parameters, the run, the stores back.
// Takes over the session.
static int run_and_fetch_chains(gpt_sgld_session* s, const gpt_sgld_config* cfg, int32_t nchains,
                                const double* epsw, const double* epsU, const double* signal_var,
                                double* const* w_store, double* const* U_store, int32_t* status) {
  SessionGuard guard(s, gpt_sgld_session_destroy);
  if (epsw || epsU || signal_var)
    for (int c = 0; c < nchains; ++c)
      GPT_TRY(gpt_sgld_session_set_hyper(s, c, epsw ? epsw[c] : cfg->epsw, epsU ? epsU[c] : cfg->epsU,
                                         signal_var ? signal_var[c] : cfg->signal_var, cfg->sigma_w));
  GPT_TRY(gpt_sgld_session_run(s, session_run_info(s).total_steps));
  for (int c = 0; c < nchains; ++c)
    GPT_TRY(gpt_sgld_session_fetch(s, c, w_store ? w_store[c] : nullptr,
                                   U_store ? U_store[c] : nullptr, nullptr, &status[c]));
  return GPT_OK;
}

// Independent chains from host arrays through one device session (the chain / wave engines that
// the device-pointer session API reaches): kin40kExperiment.jl:67-74's sweep block, every sweep
// its own phi and hyper-parameters, or posterior chains on one phi.  Each distinct phi / y array is
// copied to the device once (the pointers may repeat).
extern "C" int gpt_sgld_regression_chains(const gpt_sgld_config* cfg, int32_t nchains,
                                          const uint64_t* seeds, const double* const* phi,
                                          const double* const* y, const int32_t* I,
                                          const double* epsw, const double* epsU,
                                          const double* signal_var, double* const* w_store,
                                          double* const* U_store, int32_t* status) {
  if (!valid_cfg(cfg)) return GPT_ERR_BAD_DIMS;
  if (nchains < 1 || !seeds || !phi || !y || !I || !status) {
    set_error("gpt_sgld_regression_chains: null or empty arguments");
    return GPT_ERR_BAD_DIMS;
  }
  const bool stores = w_store || U_store;
  for (int c = 0; c < nchains; ++c) {
    if (!phi[c] || !y[c] || (w_store && !w_store[c]) || (U_store && !U_store[c])) {
      set_error("gpt_sgld_regression_chains: null per-chain pointer");
      return GPT_ERR_BAD_DIMS;
    }
  }
  const size_t nphi = (size_t)cfg->n * cfg->D * cfg->N;
  UploadCache uc;
  std::vector<const double*> dphi(nchains), dy(nchains);
  for (int c = 0; c < nchains; ++c) {
    GPT_HIPCHK(upload_once(uc, phi[c], nphi, &dphi[c]));
    GPT_HIPCHK(upload_once(uc, y[c], (size_t)cfg->N, &dy[c]));
  }
  gpt_sgld_session* s = nullptr;
  GPT_TRY(gpt_sgld_session_create(cfg, nchains, seeds, dphi.data(), dy.data(), I,
                                  stores ? kFlagStore : 0, nullptr, &s));
  return run_and_fetch_chains(s, cfg, nchains, epsw, epsU, signal_var, w_store, U_store, status);
}

// gpt_sgld_regression_chains from X: the sweep block of kin40kExperiment.jl:67-74 with every sweep's
// features formed on the device from the shared X, Z, b and its own length scales and sigma_RBF
// (an X session), so the host neither computes nor uploads a phi.
extern "C" int gpt_sgld_regression_chains_x(const gpt_sgld_config* cfg, int32_t nchains,
                                            const uint64_t* seeds, const double* X,
                                            const double* const* y, const double* length_scale,
                                            int64_t ls_len, const double* sigma_rbf,
                                            double phi_scale, const double* Z, const double* b,
                                            const int32_t* I, const double* epsw,
                                            const double* epsU, const double* signal_var,
                                            double* const* w_store, double* const* U_store,
                                            int32_t* status) {
  if (!status) { set_error("gpt_sgld_regression_chains_x: null status"); return GPT_ERR_BAD_DIMS; }
  const bool stores = w_store || U_store;
  if (!valid_x_args(cfg, nchains, seeds, X, y, length_scale, ls_len, sigma_rbf, Z, b, I,
                    stores ? kFlagStore : 0))
    return GPT_ERR_BAD_DIMS;
  for (int c = 0; c < nchains; ++c)
    if ((w_store && !w_store[c]) || (U_store && !U_store[c])) {
      set_error("gpt_sgld_regression_chains_x: null per-chain pointer");
      return GPT_ERR_BAD_DIMS;
    }
  {
    std::vector<int32_t> I0;                    // checked here, before the uploads
    if (!zero_based_I(I, cfg->Q, cfg->D, cfg->r, I0)) return GPT_ERR_BAD_DIMS;
  }
  const size_t N = (size_t)cfg->N, D = (size_t)cfg->D, n = (size_t)cfg->n;
  UploadCache uc;
  const double *dX = nullptr, *dZ = nullptr, *db = nullptr, *dls = nullptr;
  GPT_HIPCHK(upload_once(uc, X, N * D, &dX));
  GPT_HIPCHK(upload_once(uc, Z, n * D, &dZ));
  GPT_HIPCHK(upload_once(uc, b, n * D, &db));
  GPT_HIPCHK(upload_once(uc, length_scale, (size_t)ls_len * nchains, &dls));
  std::vector<const double*> dy(nchains);
  for (int c = 0; c < nchains; ++c) GPT_HIPCHK(upload_once(uc, y[c], N, &dy[c]));
  gpt_sgld_session* s = nullptr;
  GPT_TRY(gpt_sgld_session_create_x(cfg, nchains, seeds, dX, dy.data(), dls, ls_len, sigma_rbf,
                                    phi_scale, dZ, db, I, stores ? kFlagStore : 0, nullptr, &s));
  return run_and_fetch_chains(s, cfg, nchains, epsw, epsU, signal_var, w_store, U_store, status);
}

extern "C" int gpt_sgld_rmsprop(const gpt_sgld_config* cfg, double epsilon, double alpha,
                                const double* phi, const double* y, const int32_t* I,
                                const double* w_init, const double* U_init, double* w_store,
                                double* U_store, double* diag) {
  if (!(epsilon > 0)) { set_error("RMSprop needs epsilon > 0"); return GPT_ERR_BAD_DIMS; }
  return host_sampler(cfg, phi, y, I, w_init, U_init, w_store, U_store, diag, kFlagGrid, epsilon,
                      alpha);
}

extern "C" int gpt_sgld_wonly(const gpt_sgld_config* cfg, const double* phi, const double* y,
                              const int32_t* I, const double* w_init, const double* U_init,
                              double* w_store, double* U_out, double* diag) {
  if (!cfg || !cfg->stiefel || !cfg->langevin) {
    set_error("GPT_SGLDERMw: U is a uniform Stiefel draw and w takes SGLD steps (stiefel = langevin = 1)");
    return GPT_ERR_BAD_DIMS;
  }
  return host_sampler(cfg, phi, y, I, w_init, U_init, w_store, nullptr, diag, kFlagWonly, 0.0, 0.0,
                      U_out);
}

extern "C" int gpt_gpnt_sgld(const double* phi, const double* y, int64_t n, int64_t N,
                             double signal_var, double sigma_theta, int64_t m, double eps_theta,
                             double decay_rate, int64_t burnin, int64_t maxepoch, uint64_t seed,
                             double* theta_store) {
  if (!phi || !y || !theta_store || n < 1 || N < 1 || m < 1 || burnin < 0 || maxepoch < 0) {
    set_error("bad GPNT_SGLD arguments"); return GPT_ERR_BAD_DIMS;
  }
  const long long nb = (N + m - 1) / m;
  const int epochs = (int)(burnin + maxepoch);
  const long long total = (long long)epochs * nb;
  std::vector<double> th0(n);
  for (int64_t j = 0; j < n; ++j) th0[j] = sigma_theta * host_normal(seed, (uint32_t)j, 0, kThetaInit, 0);
  std::vector<int32_t> ord((size_t)epochs * N);
  host_epoch_orders((int)N, seed, epochs, ord.data());
  DevMem dphi, dy, dord, dth, dst, dstat, dtb;
  GPT_HIPCHK(dphi.upload(phi, (size_t)n * N));
  GPT_HIPCHK(dy.upload(y, (size_t)N));
  GPT_HIPCHK(dord.upload(ord.data(), ord.size()));
  GPT_HIPCHK(dth.upload(th0.data(), th0.size()));
  GPT_HIPCHK(dst.alloc<double>((size_t)n * total));
  GPT_HIPCHK(dstat.alloc<int32_t>(1));
  GPT_HIPCHK(dstat.zero());
  GPT_HIPCHK(dtb.alloc<long long>(1));
  GPT_HIPCHK(dtb.zero());
  for (long long t = 0; t < total; ++t) {
    hipError_t e = launch_gpnt(dphi.as<double>(), dy.as<double>(), dord.as<int32_t>(), (int)n, (int)N,
                               (int)m, (int)nb, total, signal_var, sigma_theta, eps_theta, decay_rate,
                               seed, dth.as<double>(), dst.as<double>(), dstat.as<int32_t>(),
                               dtb.as<long long>(), (int)t, nullptr);
    if (e != hipSuccess) return hip_fail(e, "gpnt kernel");
  }
  int32_t st = 0;
  GPT_HIPCHK(dstat.download(&st, 1));
  if (st) {
    std::memset(theta_store, 0, 8 * (size_t)n * total);
    set_error("Get NaN in theta. Try smaller epsilon");
    return GPT_ERR_NAN_THETA;
  }
  GPT_HIPCHK(dst.download(theta_store, (size_t)n * total));
  return GPT_OK;
}
