// Classification from host arrays: GPTclassification on a session of class chains, GPNT_SGLDclass
// and the evaluation of class scores (miss rate, negative log probability).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "eval_frame.h"

using namespace gpt;

// Smallest and largest of the N >= 1 class labels; false when a label is not an integer.
static bool label_range(const double* y, int64_t N, double* lo, double* hi) {
  bool ints = true;
  *lo = *hi = y[0];
  for (int64_t i = 0; i < N; ++i) {
    ints = ints && y[i] == std::floor(y[i]);
    *lo = std::min(*lo, y[i]);
    *hi = std::max(*hi, y[i]);
  }
  return ints;
}

extern "C" int gpt_sgld_classification(const gpt_sgld_config* cfg, const double* phi,
                                       const double* y, const int32_t* I, const double* w_init,
                                       const double* U_init, double* w_store, double* U_store,
                                       double* diag) {
  if (!valid_cfg(cfg)) return GPT_ERR_BAD_DIMS;
  if (!phi || !y || !I) { set_error("null input"); return GPT_ERR_BAD_DIMS; }
  const int64_t N = cfg->N, Q = cfg->Q, nur = cfg->n * cfg->r * cfg->D;
  double lo = 0.0, hi = 0.0;
  if (!label_range(y, N, &lo, &hi)) { set_error("class labels must be integers"); return GPT_ERR_BAD_DIMS; }
  if (lo != 1 || hi > 64) {
    set_error("class labels must be 1..C (C <= 64): they index the classes (GPT_SGLD.jl:520)");
    return GPT_ERR_BAD_DIMS;
  }
  const int ncls = (int)hi;
  DevMem dphi, dy;
  GPT_HIPCHK(dphi.upload(phi, (size_t)cfg->n * cfg->D * N));
  GPT_HIPCHK(dy.upload(y, (size_t)N));
  std::vector<uint64_t> seeds(ncls, cfg->seed);
  std::vector<const double*> pp(ncls, dphi.as<double>()), yy(ncls, dy.as<double>());
  gpt_sgld_session* s = nullptr;
  const int flags = ((w_store || U_store) ? kFlagStore : 0) | (diag ? kFlagDiag : 0) | kFlagCls;
  GPT_TRY(gpt_sgld_session_create(cfg, ncls, seeds.data(), pp.data(), yy.data(), I, flags, nullptr, &s));
  std::unique_ptr<gpt_sgld_session, void (*)(gpt_sgld_session*)> guard(s, gpt_sgld_session_destroy);
  GPT_TRY(session_alloc_aux(s));
  std::vector<double> w0((size_t)Q), U0((size_t)nur);
  for (int c = 0; c < ncls; ++c) {
    GPT_TRY(gpt_sgld_session_set_hyper(s, c, cfg->epsw, cfg->epsU, 1.0, 1.0));   // no noise variance
    if (w_init && U_init) {
      GPT_TRY(session_set_state(s, c, w_init + (size_t)Q * c, U_init + (size_t)nur * c));
    } else {
      host_init_state((int)cfg->n, (int)cfg->r, (int)cfg->D, (int)Q, cfg->seed, cfg->stiefel != 0,
                      1.0, w0.data(), U0.data(), c, true);
      GPT_TRY(session_set_state(s, c, w0.data(), U0.data()));
    }
  }
  const SessionRun run = session_run_info(s);
  GPT_TRY(gpt_sgld_session_run(s, run.total_steps));
  const int64_t T = run.nstore, steps = run.total_steps;
  std::vector<double> wb(w_store ? (size_t)Q * T : 0), Ub(U_store ? (size_t)nur * T : 0),
      db(diag ? (size_t)(1 + cfg->D) * steps : 0);
  bool bad = false;
  for (int c = 0; c < ncls; ++c) {
    int32_t st = 0;
    GPT_TRY(gpt_sgld_session_fetch(s, c, w_store ? wb.data() : nullptr, U_store ? Ub.data() : nullptr,
                                   diag ? db.data() : nullptr, &st));
    bad |= st != 0;
    for (int64_t z = 0; z < T; ++z) {      // (Q, C, T) and (n, r, D, C, T) column-major
      if (w_store) std::memcpy(w_store + ((size_t)z * ncls + c) * Q, wb.data() + (size_t)z * Q, 8 * Q);
      if (U_store) std::memcpy(U_store + ((size_t)z * ncls + c) * nur, Ub.data() + (size_t)z * nur, 8 * nur);
    }
    if (diag) std::memcpy(diag + (size_t)c * db.size(), db.data(), 8 * db.size());
  }
  if (bad) {                               // GPT_SGLD.jl:632-634: zero stores
    if (w_store) std::memset(w_store, 0, 8 * (size_t)Q * ncls * T);
    if (U_store) std::memset(U_store, 0, 8 * (size_t)nur * ncls * T);
    set_error("Get NaN when moving along Geodesic. Try smaller epsU");
    return GPT_ERR_NAN_GEODESIC;
  }
  return GPT_OK;
}

// Device-event times of the last classification calls on this thread (gpt_class_last_timing):
// [0] the sampler's launches, [1] the scores (nt_scores_kernel or the stacked prediction),
// [2] the evaluation kernels.
static thread_local double g_cls_ms[3] = {0.0, 0.0, 0.0};
extern "C" int gpt_class_last_timing(double* ms_out) {
  if (!ms_out) { set_error("gpt_class_last_timing: null argument"); return GPT_ERR_BAD_DIMS; }
  for (int k = 0; k < 3; ++k) ms_out[k] = g_cls_ms[k];
  return GPT_OK;
}

// GPNT_SGLDclass (GPT_SGLD.jl:851-901) for sibling chains on one phi / y: chain k draws
// theta[:, c] = sigma_theta·normals(n, seeds[k], 0, THETA_INIT, c), its epoch orders are
// GPNT_SGLD's for seeds[k], and the kernel draws the step noise (cls.hip).  One launch per epoch.
extern "C" int gpt_gpnt_sgld_class_chains(const double* phi, const double* y, int64_t n, int64_t N,
                                          int64_t ncls, double sigma_theta, int64_t m,
                                          const double* eps_theta, double decay_rate,
                                          int64_t burnin, int64_t maxepoch, const uint64_t* seeds,
                                          int32_t nchains, int64_t store_every, double* theta_store,
                                          int32_t* status) {
  if (!phi || !y || !eps_theta || !seeds || !theta_store || !status) {
    set_error("gpt_gpnt_sgld_class_chains: null argument"); return GPT_ERR_BAD_DIMS;
  }
  // m <= 2^20, not 2^31 - 1: the C·m residual and the staged n·m features are sized by m, not min(m, N)
  if (!theta_chain_dims_ok(n, N, m, burnin, maxepoch, nchains, store_every) || m > (1 << 20)) {
    set_error("bad GPNT_SGLDclass dimensions"); return GPT_ERR_BAD_DIMS;
  }
  if (ncls < 1 || ncls > 32) {
    set_error("GPNT_SGLDclass: the number of classes must be in 1..32"); return GPT_ERR_BAD_DIMS;
  }
  const int C = (int)ncls;
  double lo = 0.0, hi = 0.0;
  if (!label_range(y, N, &lo, &hi) || !(lo >= 1.0 && hi <= (double)C)) {
    set_error("GPNT_SGLDclass: labels must be integers in 1..C"); return GPT_ERR_BAD_DIMS;
  }
  std::vector<int32_t> y0((size_t)N);
  for (int64_t i = 0; i < N; ++i) y0[i] = (int32_t)y[i] - 1;
  const NtcLayout L = ntc_layout((int)n, C, (int)m);
  if (L.bytes > (size_t)kMaxLds) {
    set_error("GPNT_SGLDclass: theta (n x C) and the batch residual exceed 160 KiB of LDS");
    return GPT_ERR_BAD_DIMS;
  }
  const ThetaRun R(N, m, burnin, maxepoch, store_every);
  for (int k = 0; k < nchains; ++k) status[k] = 0;
  if (R.total == 0) return GPT_OK;
  ThetaChainSet S;
  GPT_TRY(S.init(seeds, eps_theta, nchains, n, C, N, R, &sigma_theta, 0));
  std::vector<NtcChain> ch(nchains);
  for (int k = 0; k < nchains; ++k) ch[k] = NtcChain{S.chain(k)};
  DevMem dphi, dy, dch;
  GPT_HIPCHK(dphi.upload(phi, (size_t)n * N));
  GPT_HIPCHK(dy.upload(y0.data(), y0.size()));
  GPT_HIPCHK(dch.upload(ch.data(), ch.size()));
  return S.run(R, &g_cls_ms[0], "ntc_chain kernel", [&](long long t0, int nsteps) {
    return launch_ntc_chain(dphi.as<double>(), dy.as<int32_t>(), dch.as<NtcChain>(), nchains,
                            (int)n, (int)N, C, (int)m, (int)R.nb, R.total, decay_rate,
                            (int)store_every, t0, nsteps, L, nullptr);
  }, theta_store, status);
}

extern "C" int gpt_gpnt_sgld_class(const double* phi, const double* y, int64_t n, int64_t N,
                                   double sigma_theta, int64_t m, double eps_theta,
                                   double decay_rate, int64_t burnin, int64_t maxepoch,
                                   uint64_t seed, double* theta_store) {
  if (!phi || !y || !theta_store || N < 1) {
    set_error("bad GPNT_SGLDclass arguments"); return GPT_ERR_BAD_DIMS;
  }
  double lo = 0.0, hi = 0.0;
  (void)label_range(y, N, &lo, &hi);                          // integers: checked by the chains entry
  const double Cd = hi - lo + 1.0;                            // :854
  if (!(Cd >= 1.0 && Cd <= 32.0)) {
    set_error("GPNT_SGLDclass: C = max(y) - min(y) + 1 must be in 1..32"); return GPT_ERR_BAD_DIMS;
  }
  int32_t st = 0;
  GPT_TRY(gpt_gpnt_sgld_class_chains(phi, y, n, N, (int64_t)Cd, sigma_theta, m, &eps_theta,
                                     decay_rate, burnin, maxepoch, &seed, 1, 1, theta_store, &st));
  if (st) { set_error("Get NaN in theta. Try smaller epsilon"); return GPT_ERR_NAN_THETA; }
  return GPT_OK;
}

// Evaluation of device scores (Ntest, C, T) against device labels; every output is a device
// pointer, the last three optional.  Synchronises st (the workspace is freed on return).
static int class_eval_core(const double* scores, const int32_t* y, int64_t Ntest, int64_t C,
                           int64_t T, int64_t avg_first, int64_t avg_last, double* prop_missed,
                           double* mean_nlp, double* avg, double* mean_scores, int32_t* prediction,
                           double* nlp, hipStream_t st) {
  const size_t ntiles = class_eval_tiles(Ntest);
  DevMem dpn, dpm, dms;
  GPT_HIPCHK(dpn.alloc<double>(ntiles * (size_t)T));
  GPT_HIPCHK(dpm.alloc<int32_t>(ntiles * (size_t)T));
  if (!mean_scores) {
    GPT_HIPCHK(dms.alloc<double>((size_t)Ntest * C));
    mean_scores = dms.as<double>();
  }
  EventTimer tm(&g_cls_ms[2], st);
  hipError_t e = launch_class_eval(scores, y, Ntest, (int)C, (int)T, dpn.as<double>(),
                                   dpm.as<int32_t>(), prop_missed, mean_nlp, nullptr, nullptr, st);
  if (e != hipSuccess) return hip_fail(e, "class_eval kernel");
  e = launch_class_mean(scores, Ntest, (int)C, (int)avg_first, (int)avg_last, mean_scores, st);
  if (e != hipSuccess) return hip_fail(e, "class_mean kernel");
  e = launch_class_eval(mean_scores, y, Ntest, (int)C, 1, dpn.as<double>(), dpm.as<int32_t>(), avg,
                        avg + 1, prediction, nlp, st);
  if (e != hipSuccess) return hip_fail(e, "class_eval kernel");
  tm.stop();
  GPT_HIPCHK(hipStreamSynchronize(st));
  return GPT_OK;
}

static bool valid_class_eval(const void* scores, const void* ytest, int64_t Ntest, int64_t C,
                             int64_t T, int64_t avg_first, int64_t avg_last, const void* pm,
                             const void* nl, const void* avg) {
  if (!scores || !ytest || !pm || !nl || !avg) { set_error("class_eval: null argument"); return false; }
  if (Ntest < 1 || C < 1 || T < 1 || C > (1 << 20) || T > (1 << 24) || Ntest > (1LL << 40)) {
    set_error("class_eval: bad dimensions"); return false;
  }
  return window_ok("class_eval", "avg_", avg_first, avg_last, T);
}

static bool valid_labels(const int32_t* y, int64_t Ntest, int64_t C) {
  for (int64_t i = 0; i < Ntest; ++i)
    if (y[i] < 1 || y[i] > C) { set_error("class_eval: labels must be in 1..C"); return false; }
  return true;
}

extern "C" int gpt_class_eval_dev(const double* scores_dev, const int32_t* ytest_dev, int64_t Ntest,
                                  int64_t C, int64_t T, int64_t avg_first, int64_t avg_last,
                                  double* prop_missed_dev, double* mean_nlp_dev, double* avg_dev,
                                  double* mean_scores_dev, int32_t* prediction_dev, double* nlp_dev,
                                  void* hip_stream) {
  if (!valid_class_eval(scores_dev, ytest_dev, Ntest, C, T, avg_first, avg_last, prop_missed_dev,
                        mean_nlp_dev, avg_dev))
    return GPT_ERR_BAD_DIMS;
  std::vector<int32_t> yh((size_t)Ntest);                     // the labels are checked on the host
  GPT_HIPCHK(hipMemcpyAsync(yh.data(), ytest_dev, 4 * (size_t)Ntest, hipMemcpyDeviceToHost,
                            (hipStream_t)hip_stream));
  GPT_HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
  if (!valid_labels(yh.data(), Ntest, C)) return GPT_ERR_BAD_DIMS;
  return class_eval_core(scores_dev, ytest_dev, Ntest, C, T, avg_first, avg_last, prop_missed_dev,
                         mean_nlp_dev, avg_dev, mean_scores_dev, prediction_dev, nlp_dev,
                         (hipStream_t)hip_stream);
}

// The evaluation of device scores (Ntest, C, T) into host outputs (ytest already checked); the
// scores themselves come back too when asked for.
static int class_eval_to_host(const double* dscores, const int32_t* ytest, int64_t Ntest, int64_t C,
                              int64_t T, int64_t avg_first, int64_t avg_last, double* prop_missed,
                              double* mean_nlp, double* avg, double* mean_scores,
                              int32_t* prediction, double* nlp, double* scores_out) {
  DevMem dy, dpm, dnl, davg, dms, dpr, dnp;
  GPT_HIPCHK(dy.upload(ytest, (size_t)Ntest));
  GPT_HIPCHK(dpm.alloc<double>((size_t)T));
  GPT_HIPCHK(dnl.alloc<double>((size_t)T));
  GPT_HIPCHK(davg.alloc<double>(2));
  GPT_HIPCHK(dms.alloc<double>((size_t)Ntest * C));
  GPT_HIPCHK(dpr.alloc<int32_t>((size_t)Ntest));
  GPT_HIPCHK(dnp.alloc<double>((size_t)Ntest));
  GPT_TRY(class_eval_core(dscores, dy.as<int32_t>(), Ntest, C, T, avg_first, avg_last,
                          dpm.as<double>(), dnl.as<double>(), davg.as<double>(), dms.as<double>(),
                          dpr.as<int32_t>(), dnp.as<double>(), nullptr));
  GPT_HIPCHK(dpm.download(prop_missed, (size_t)T));
  GPT_HIPCHK(dnl.download(mean_nlp, (size_t)T));
  GPT_HIPCHK(davg.download(avg, 2));
  if (mean_scores) GPT_HIPCHK(dms.download(mean_scores, (size_t)Ntest * C));
  if (prediction) GPT_HIPCHK(dpr.download(prediction, (size_t)Ntest));
  if (nlp) GPT_HIPCHK(dnp.download(nlp, (size_t)Ntest));
  if (scores_out)
    GPT_HIPCHK(hipMemcpy(scores_out, dscores, 8 * (size_t)Ntest * C * T, hipMemcpyDeviceToHost));
  return GPT_OK;
}

extern "C" int gpt_class_eval(const double* scores, const int32_t* ytest, int64_t Ntest, int64_t C,
                              int64_t T, int64_t avg_first, int64_t avg_last,
                              double* prop_missed_out, double* mean_nlp_out, double* avg_out,
                              double* mean_scores_out, int32_t* prediction_out, double* nlp_out) {
  if (!valid_class_eval(scores, ytest, Ntest, C, T, avg_first, avg_last, prop_missed_out,
                        mean_nlp_out, avg_out) || !valid_labels(ytest, Ntest, C))
    return GPT_ERR_BAD_DIMS;
  DevMem ds;
  GPT_HIPCHK(ds.upload(scores, (size_t)Ntest * C * T));
  return class_eval_to_host(ds.as<double>(), ytest, Ntest, C, T, avg_first, avg_last,
                            prop_missed_out, mean_nlp_out, avg_out, mean_scores_out, prediction_out,
                            nlp_out, nullptr);
}

// ImageNoTensorExperiment.jl:50-75 on T stored full-theta samples: scores = phitestᵀ·theta for
// every (class, sample) in one launch, then the evaluation.
extern "C" int gpt_gpnt_pred_class(const double* theta, const double* phitest, const int32_t* ytest,
                                   int64_t n, int64_t Ntest, int64_t C, int64_t T,
                                   int64_t avg_first, int64_t avg_last, double* prop_missed_out,
                                   double* mean_nlp_out, double* avg_out, double* mean_scores_out,
                                   int32_t* prediction_out, double* nlp_out, double* scores_out) {
  if (!theta || !phitest || n < 1 || n > (1 << 24)) {
    set_error("gpt_gpnt_pred_class: bad arguments"); return GPT_ERR_BAD_DIMS;
  }
  if (!valid_class_eval(theta, ytest, Ntest, C, T, avg_first, avg_last, prop_missed_out,
                        mean_nlp_out, avg_out) || !valid_labels(ytest, Ntest, C))
    return GPT_ERR_BAD_DIMS;
  if ((C * T + 63) / 64 > 65535) { set_error("gpt_gpnt_pred_class: C*T too large"); return GPT_ERR_BAD_DIMS; }
  ThetaScores sc{n, Ntest, C * T};
  DevMem dphi;
  GPT_TRY(sc.stage(theta));
  GPT_HIPCHK(dphi.upload(phitest, (size_t)n * Ntest));
  {
    EventTimer tm(&g_cls_ms[1], nullptr);
    GPT_TRY(sc.launch(dphi.as<double>()));
    tm.stop();
  }
  return class_eval_to_host(sc.s.as<double>(), ytest, Ntest, C, T, avg_first, avg_last,
                            prop_missed_out, mean_nlp_out, avg_out, mean_scores_out, prediction_out,
                            nlp_out, scores_out);
}

// ImageExperiment.jl:50-72 on T stored samples of GPTclassification: w (Q, C, T) and
// U (n, r, D, C, T) are S = C·T stacked samples in (c, t) order, so launch_pred's fhat (Ntest, S)
// (pred_store_fhat, as gpt_pred_mean's) is the scores array; phitest is uploaded once.
extern "C" int gpt_pred_class(const double* w, const double* U, const int32_t* I,
                              const double* phitest, const int32_t* ytest, int64_t n, int64_t D,
                              int64_t Ntest, int64_t r, int64_t Q, int64_t C, int64_t T,
                              int64_t avg_first, int64_t avg_last, double* prop_missed_out,
                              double* mean_nlp_out, double* avg_out, double* mean_scores_out,
                              int32_t* prediction_out, double* nlp_out, double* scores_out) {
  if (!w || !U || !I || !phitest) { set_error("gpt_pred_class: null argument"); return GPT_ERR_BAD_DIMS; }
  if (!valid_pred(n, D, Ntest, r, Q)) return GPT_ERR_BAD_DIMS;
  if (!valid_class_eval(w, ytest, Ntest, C, T, avg_first, avg_last, prop_missed_out, mean_nlp_out,
                        avg_out) || !valid_labels(ytest, Ntest, C))
    return GPT_ERR_BAD_DIMS;
  if (C * T > (1LL << 30)) { set_error("gpt_pred_class: C*T too large"); return GPT_ERR_BAD_DIMS; }
  DevMem ds;
  GPT_TRY(pred_store_fhat(w, U, I, phitest, n, D, Ntest, r, Q, C * T, ds, &g_cls_ms[1]));
  return class_eval_to_host(ds.as<double>(), ytest, Ntest, C, T, avg_first, avg_last,
                            prop_missed_out, mean_nlp_out, avg_out, mean_scores_out, prediction_out,
                            nlp_out, scores_out);
}
