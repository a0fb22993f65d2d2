// The joint likelihood of the full-theta softmax classifier from host arrays: the resident
// evaluator gpt_cjoint (value, gradient, Langevin steps and HMC transitions on theta, scores of
// test rows) and the one-shot entries.  The kernels are in cjoint.hip and chmc.hip.
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "gp_handle.h"

using namespace gpt;

struct gpt_cjoint {
  int n = 0, D = 0, C = 0;
  long long N = 0;
  CjLayout L;
  double *X = nullptr, *Z = nullptr, *b = nullptr, *ls = nullptr, *theta = nullptr,
         *part_theta = nullptr, *part_tx = nullptr, *part_sc = nullptr, *out = nullptr;
  int32_t *y0 = nullptr, *status = nullptr;
  int64_t step = 0;                   // 0-based counter of the next Langevin step / HMC transition
  // HMC (chmc.hip), allocated by the first call that needs it.  cache: sc[0] and g_cur hold U
  // and grad U of the resident theta at these hyper-parameters (compared by bits).
  HmcDev hmc = {};
  bool hmc_alloc = false;
  FactorKey cache;
  DevSet mem;
};

static bool cj_dims_ok(const void* X, int64_t N, int64_t D, int64_t C, const void* Z, const void* b,
                       int64_t n) {
  if (!X || !Z || !b) { set_error("cjoint: null input array"); return false; }
  if (n < 1 || n > 1024) { set_error("cjoint: n must be in 1..1024"); return false; }
  if (N < 1 || N > (1LL << 31) - 1) { set_error("cjoint: N must be in 1..2^31-1"); return false; }
  if (D < 1 || D > kDMax) { set_error("cjoint: D must be in 1..16"); return false; }
  if (C < 1 || C > 32) { set_error("cjoint: the number of classes must be in 1..32"); return false; }
  return true;
}

static bool cj_hyper_ok(const double* hyper, int64_t Lh, int64_t D) {
  return hyper_ok("cjoint", hyper, Lh, D, 1);
}

extern "C" int gpt_cjoint_create(const double* X, int64_t N, int64_t D, const double* y, int64_t C,
                                 const double* Z, const double* b, int64_t n, gpt_cjoint** out) {
  if (!out) { set_error("cjoint: null handle pointer"); return GPT_ERR_BAD_DIMS; }
  *out = nullptr;
  if (!cj_dims_ok(X, N, D, C, Z, b, n)) return GPT_ERR_BAD_DIMS;
  if (!y) { set_error("cjoint: null input array"); return GPT_ERR_BAD_DIMS; }
  std::vector<int32_t> y0((size_t)N);
  for (int64_t i = 0; i < N; ++i) {
    if (!(y[i] == std::floor(y[i])) || !(y[i] >= 1.0 && y[i] <= (double)C)) {
      set_error("cjoint: labels must be integers in 1..C"); return GPT_ERR_BAD_DIMS;
    }
    y0[i] = (int32_t)y[i] - 1;
  }
  std::unique_ptr<gpt_cjoint> h(new gpt_cjoint);
  h->n = (int)n; h->D = (int)D; h->C = (int)C; h->N = N;
  h->L = cjoint_layout((int)n, N, (int)C);
  DevSet& M = h->mem;
  const size_t nC = (size_t)n * C, nb = (size_t)h->L.nblk;
  GPT_HIPCHK(M.upload(&h->X, X, (size_t)N * D));
  GPT_HIPCHK(M.upload(&h->y0, (const int32_t*)y0.data(), (size_t)N));
  GPT_HIPCHK(M.upload(&h->Z, Z, (size_t)n * D));
  GPT_HIPCHK(M.upload(&h->b, b, (size_t)n));
  GPT_HIPCHK(M.alloc(&h->ls, (size_t)kDMax));
  GPT_HIPCHK(M.alloc(&h->theta, nC));
  GPT_HIPCHK(M.alloc(&h->part_theta, nb * nC));
  GPT_HIPCHK(M.alloc(&h->part_tx, nb * (size_t)n * D));
  GPT_HIPCHK(M.alloc(&h->part_sc, 2 * nb));
  GPT_HIPCHK(M.alloc(&h->out, 2 + (size_t)D + nC));
  GPT_HIPCHK(M.alloc(&h->status, 4));
  GPT_HIPCHK(hipMemset(h->theta, 0, 8 * nC));
  GPT_HIPCHK(hipMemset(h->status, 0, 16));
  *out = h.release();
  return GPT_OK;
}

extern "C" int gpt_cjoint_destroy(gpt_cjoint* h) { return destroy_handle(h); }

extern "C" int gpt_cjoint_set_theta(gpt_cjoint* h, const double* theta) {
  if (!h || !theta) { set_error("cjoint: null handle or theta"); return GPT_ERR_BAD_DIMS; }
  h->cache.clear();
  GPT_HIPCHK(hipMemcpy(h->theta, theta, 8 * (size_t)h->n * h->C, hipMemcpyHostToDevice));
  return GPT_OK;
}

extern "C" int gpt_cjoint_get_theta(gpt_cjoint* h, double* theta_out) {
  if (!h || !theta_out) { set_error("cjoint: null handle or output"); return GPT_ERR_BAD_DIMS; }
  GPT_HIPCHK(hipMemcpy(theta_out, h->theta, 8 * (size_t)h->n * h->C, hipMemcpyDeviceToHost));
  return GPT_OK;
}

extern "C" int gpt_cjoint_steps(gpt_cjoint* h, int64_t* step_out) {
  if (!h || !step_out) { set_error("cjoint: null handle or output"); return GPT_ERR_BAD_DIMS; }
  *step_out = h->step;
  return GPT_OK;
}

// The kernel arguments at hyper (the length scales go to the device); sigma_out = sigma_RBF.
static int cj_args(gpt_cjoint* h, const double* hyper, int64_t Lh, hipStream_t st, CjArgs* A,
                   double* sigma_out) {
  const int D = h->D;
  double lsv[kDMax];
  length_scales(hyper, Lh, D, 1, lsv);
  const double sigma = hyper[Lh - 1];
  GPT_HIPCHK(hipMemcpyAsync(h->ls, lsv, 8 * (size_t)D, hipMemcpyHostToDevice, st));
  GPT_HIPCHK(hipStreamSynchronize(st));               // lsv is on this frame
  A->X = h->X; A->N = h->N; A->D = D; A->n = h->n; A->C = h->C;
  A->y0 = h->y0; A->Z = h->Z; A->b = h->b; A->ls = h->ls;
  A->c = std::sqrt(2.0 / (double)h->n) * sigma;
  A->theta = h->theta;
  A->part_theta = h->part_theta; A->part_tx = h->part_tx; A->part_sc = h->part_sc;
  A->scores = nullptr;
  A->status = nullptr;
  *sigma_out = sigma;
  return GPT_OK;
}

extern "C" int gpt_cjoint_eval(gpt_cjoint* h, const double* hyper, int64_t Lh, const double* theta,
                               int32_t want_grad, double* value, double* grad_theta,
                               double* grad_hyper) {
  if (!h || !value) { set_error("cjoint: null handle or output"); return GPT_ERR_BAD_DIMS; }
  if (!cj_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  if (theta) {
    const int rc = gpt_cjoint_set_theta(h, theta);
    if (rc != GPT_OK) return rc;
  }
  hipStream_t st = nullptr;
  CjArgs A;
  double sigma = 0.0;
  int rc = cj_args(h, hyper, Lh, st, &A, &sigma);
  if (rc != GPT_OK) return rc;
  const bool full = want_grad != 0;
  GPT_HIPCHK(launch_cjoint_eval(A, h->L, full ? kCjFull : kCjValue, st));
  GPT_HIPCHK(launch_cjoint_finish(A, h->L, sigma, full, h->out, st));
  const int D = h->D;
  const size_t nC = (size_t)h->n * h->C;
  double head[2 + kDMax];
  GPT_HIPCHK(hipMemcpy(head, h->out, 8 * (size_t)(full ? 2 + D : 2), hipMemcpyDeviceToHost));
  *value = head[0];
  if (full && grad_theta)
    GPT_HIPCHK(hipMemcpy(grad_theta, h->out + 2 + D, 8 * nC, hipMemcpyDeviceToHost));
  if (full && grad_hyper) {
    fold_ls_grad(head + 2, D, Lh, 1, grad_hyper);
    grad_hyper[Lh - 1] = head[1];
  }
  return GPT_OK;
}

extern "C" int gpt_cjoint_langevin(gpt_cjoint* h, const double* hyper, int64_t Lh, double eps,
                                   int64_t nsteps, uint64_t seed, int64_t t0) {
  if (!h) { set_error("cjoint: null handle"); return GPT_ERR_BAD_DIMS; }
  if (!cj_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  if (!(eps > 0.0) || nsteps < 0 || nsteps > (1 << 24)) {
    set_error("cjoint: eps must be positive and nsteps in 0..2^24"); return GPT_ERR_BAD_DIMS;
  }
  const int64_t first = t0 >= 0 ? t0 : h->step;
  if (first + nsteps > (1LL << 32)) {
    set_error("cjoint: the step counter must stay below 2^32"); return GPT_ERR_BAD_DIMS;
  }
  hipStream_t st = nullptr;
  CjArgs A;
  double sigma = 0.0;
  int rc = cj_args(h, hyper, Lh, st, &A, &sigma);
  if (rc != GPT_OK) return rc;
  GPT_HIPCHK(hipMemsetAsync(h->status, 0, 16, st));
  A.status = h->status;
  h->cache.clear();
  for (int64_t t = first; t < first + nsteps; ++t) {
    GPT_HIPCHK(launch_cjoint_eval(A, h->L, kCjTheta, st));
    GPT_HIPCHK(launch_cjoint_update(A, h->L, h->theta, eps, seed, (uint32_t)t, h->status, st));
  }
  int32_t bad = 0;
  GPT_HIPCHK(hipMemcpy(&bad, h->status, 4, hipMemcpyDeviceToHost));
  h->step = first + nsteps;
  if (bad) { set_error("Get NaN in theta. Try smaller epsilon"); return GPT_ERR_NAN_THETA; }
  return GPT_OK;
}

// ---- Hamiltonian Monte Carlo on the resident theta (chmc.hip) -----------------------------------
static int cj_hmc_buffers(gpt_cjoint* h) {
  if (h->hmc_alloc) return GPT_OK;
  DevSet& M = h->mem;
  HmcDev& S = h->hmc;
  const size_t nC = (size_t)h->n * h->C, nb = (size_t)hmc_blocks(h->n, h->C);
  GPT_HIPCHK(M.alloc(&S.q, nC));
  GPT_HIPCHK(M.alloc(&S.p, nC));
  GPT_HIPCHK(M.alloc(&S.g_cur, nC));
  GPT_HIPCHK(M.alloc(&S.g_new, nC));
  GPT_HIPCHK(M.alloc(&S.kin0, nb));
  GPT_HIPCHK(M.alloc(&S.kin1, nb));
  GPT_HIPCHK(M.alloc(&S.prior, nb));
  GPT_HIPCHK(M.alloc(&S.sc, 4));
  GPT_HIPCHK(M.alloc(&S.flag, 4));
  GPT_HIPCHK(M.alloc(&S.ndiv, 2));
  S.theta = h->theta;
  S.status = h->status;
  S.n = h->n;
  S.C = h->C;
  h->hmc_alloc = true;
  return GPT_OK;
}

static bool cj_hmc_step_ok(double eps, int64_t L) {
  if (!(eps > 0.0) || !std::isfinite(eps)) { set_error("cjoint: eps must be positive and finite"); return false; }
  if (L < 1 || L > 1024) { set_error("cjoint: the number of leapfrog steps must be in 1..1024"); return false; }
  return true;
}

// The kernel arguments at hyper, the status word cleared, and the cache of the resident theta:
// when it does not stand for this theta at these hyper bits, one evaluation at theta forms U and
// grad U, and a non-finite U (a non-finite theta makes it so) is GPT_ERR_NAN_THETA.
static int cj_hmc_prepare(gpt_cjoint* h, const double* hyper, int64_t Lh, hipStream_t st, CjArgs* A) {
  int rc = cj_hmc_buffers(h);
  if (rc != GPT_OK) return rc;
  double sigma = 0.0;
  rc = cj_args(h, hyper, Lh, st, A, &sigma);
  if (rc != GPT_OK) return rc;
  GPT_HIPCHK(hipMemsetAsync(h->status, 0, 16, st));
  A->status = h->status;
  if (h->cache.matches(hyper, Lh)) return GPT_OK;
  h->cache.clear();
  const HmcDev& S = h->hmc;
  GPT_HIPCHK(launch_cjoint_eval(*A, h->L, kCjTheta, st));
  GPT_HIPCHK(launch_hmc_prime(S, h->part_theta, h->L.nblk, st));
  GPT_HIPCHK(launch_hmc_decide(S, 0, h->part_sc, h->L.nblk, 0, 0, 0, nullptr, nullptr, nullptr, st));
  double U = 0.0;
  GPT_HIPCHK(hipMemcpy(&U, S.sc, 8, hipMemcpyDeviceToHost));
  if (!std::isfinite(U)) {
    set_error("cjoint: theta or its joint likelihood is not finite at the start of the run");
    return GPT_ERR_NAN_THETA;
  }
  h->cache.set(hyper, Lh);
  return GPT_OK;
}

// The L leapfrog steps from (theta, p): L evaluations at the work position q.
static int cj_hmc_integrate(gpt_cjoint* h, CjArgs A, double eps, int64_t L, hipStream_t st) {
  const HmcDev& S = h->hmc;
  const double s = std::sqrt(eps);
  A.theta = S.q;
  GPT_HIPCHK(launch_hmc_leap(S, 0, h->part_theta, h->L.nblk, s, st));
  for (int64_t l = 1; l <= L; ++l) {
    GPT_HIPCHK(launch_cjoint_eval(A, h->L, kCjTheta, st));
    GPT_HIPCHK(launch_hmc_leap(S, l < L ? 1 : 2, h->part_theta, h->L.nblk, s, st));
  }
  return GPT_OK;
}

extern "C" int gpt_chmc_run(gpt_cjoint* h, const double* hyper, int64_t Lh, double eps, int64_t L,
                              int64_t burnin, int64_t nsamples, int64_t thin, uint64_t seed,
                              int64_t t0, double* theta_store, int32_t* accept_out, double* dH_out,
                              double* value_out, int64_t* ndivergent_out) {
  if (!h) { set_error("cjoint: null handle"); return GPT_ERR_BAD_DIMS; }
  if (!cj_hyper_ok(hyper, Lh, h->D) || !cj_hmc_step_ok(eps, L)) return GPT_ERR_BAD_DIMS;
  if (thin < 1 || burnin < 0 || nsamples < 0 || burnin > (1 << 24) || nsamples > (1 << 24)) {
    set_error("cjoint: thin must be at least 1, burnin and nsamples in 0..2^24");
    return GPT_ERR_BAD_DIMS;
  }
  const int64_t ntrans = burnin + nsamples, first = t0 >= 0 ? t0 : h->step;
  if (first + ntrans > (1LL << 32)) {
    set_error("cjoint: the step counter must stay below 2^32"); return GPT_ERR_BAD_DIMS;
  }
  hipStream_t st = nullptr;
  CjArgs A;
  int rc = cj_hmc_prepare(h, hyper, Lh, st, &A);
  if (rc != GPT_OK) return rc;
  const HmcDev& S = h->hmc;
  const size_t nC = (size_t)h->n * h->C, ncols = (size_t)(nsamples / thin);
  const size_t nrec = ntrans > 0 ? (size_t)ntrans : 1;
  DevMem dstore, dacc, ddh, dval;
  if (theta_store) GPT_HIPCHK(dstore.alloc<double>(nC * ncols));
  GPT_HIPCHK(dacc.alloc<int32_t>(nrec));
  GPT_HIPCHK(ddh.alloc<double>(nrec));
  GPT_HIPCHK(dval.alloc<double>(nrec));
  GPT_HIPCHK(hipMemsetAsync(S.ndiv, 0, 16, st));
  h->cache.clear();                                     // until the run has gone through
  for (int64_t i = 0; i < ntrans; ++i) {
    const uint32_t t = (uint32_t)(first + i);
    GPT_HIPCHK(launch_hmc_begin(S, true, seed, t, st));
    rc = cj_hmc_integrate(h, A, eps, L, st);
    if (rc != GPT_OK) return rc;
    GPT_HIPCHK(launch_hmc_decide(S, 1, h->part_sc, h->L.nblk, seed, t, i, dacc.as<int32_t>(),
                                 ddh.as<double>(), dval.as<double>(), st));
    const int64_t k = i - burnin + 1;                   // 1-based count of transitions past burn-in
    double* col = nullptr;
    if (theta_store && k >= 1 && k % thin == 0 && (size_t)(k / thin) <= ncols)
      col = dstore.as<double>() + nC * (size_t)(k / thin - 1);
    GPT_HIPCHK(launch_hmc_commit(S, col, st));
  }
  h->step = first + ntrans;
  long long ndiv = 0;
  GPT_HIPCHK(hipMemcpy(&ndiv, S.ndiv, 8, hipMemcpyDeviceToHost));      // the one synchronisation
  if (ndivergent_out) *ndivergent_out = ndiv;
  if (theta_store && ncols) GPT_HIPCHK(dstore.download(theta_store, nC * ncols));
  if (ntrans > 0) {
    if (accept_out) GPT_HIPCHK(dacc.download(accept_out, (size_t)ntrans));
    if (dH_out) GPT_HIPCHK(ddh.download(dH_out, (size_t)ntrans));
    if (value_out) GPT_HIPCHK(dval.download(value_out, (size_t)ntrans));
  }
  h->cache.set(hyper, Lh);                              // U and grad U of the kept state stand
  return GPT_OK;
}

extern "C" int gpt_chmc_leapfrog(gpt_cjoint* h, const double* hyper, int64_t Lh, double eps,
                                   int64_t L, double* p_inout, double* q_out, double* H_out) {
  if (!h || !p_inout) { set_error("cjoint: null handle or momentum"); return GPT_ERR_BAD_DIMS; }
  if (!cj_hyper_ok(hyper, Lh, h->D) || !cj_hmc_step_ok(eps, L)) return GPT_ERR_BAD_DIMS;
  hipStream_t st = nullptr;
  CjArgs A;
  int rc = cj_hmc_prepare(h, hyper, Lh, st, &A);
  if (rc != GPT_OK) return rc;
  const HmcDev& S = h->hmc;
  const size_t nC = (size_t)h->n * h->C;
  GPT_HIPCHK(hipMemcpy(S.p, p_inout, 8 * nC, hipMemcpyHostToDevice));
  GPT_HIPCHK(launch_hmc_begin(S, false, 0, 0, st));
  rc = cj_hmc_integrate(h, A, eps, L, st);
  if (rc != GPT_OK) return rc;
  GPT_HIPCHK(launch_hmc_decide(S, 2, h->part_sc, h->L.nblk, 0, 0, 0, nullptr, nullptr, nullptr, st));
  GPT_HIPCHK(hipMemcpy(p_inout, S.p, 8 * nC, hipMemcpyDeviceToHost));
  if (q_out) GPT_HIPCHK(hipMemcpy(q_out, S.q, 8 * nC, hipMemcpyDeviceToHost));
  if (H_out) GPT_HIPCHK(hipMemcpy(H_out, S.sc + 2, 16, hipMemcpyDeviceToHost));
  return GPT_OK;
}

extern "C" int gpt_cjoint_scores_dev(gpt_cjoint* h, const double* hyper, int64_t Lh,
                                     const double* Xtest_dev, int64_t Ntest, double* scores_dev,
                                     void* hip_stream) {
  if (!h || !Xtest_dev || !scores_dev) { set_error("cjoint: null argument"); return GPT_ERR_BAD_DIMS; }
  if (Ntest < 1 || Ntest > (1LL << 31) - 1) {
    set_error("cjoint: Ntest must be in 1..2^31-1"); return GPT_ERR_BAD_DIMS;
  }
  if (!cj_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  hipStream_t st = (hipStream_t)hip_stream;
  CjArgs A;
  double sigma = 0.0;
  const int rc = cj_args(h, hyper, Lh, st, &A, &sigma);
  if (rc != GPT_OK) return rc;
  A.X = Xtest_dev; A.N = Ntest; A.y0 = nullptr; A.scores = scores_dev;
  GPT_HIPCHK(launch_cjoint_eval(A, cjoint_layout(h->n, Ntest, h->C), kCjScores, st));
  return GPT_OK;
}

extern "C" int gpt_cjoint_scores(gpt_cjoint* h, const double* hyper, int64_t Lh, const double* Xtest,
                                 int64_t Ntest, double* scores_out) {
  if (!h || !Xtest || !scores_out || Ntest < 1 || Ntest > (1LL << 31) - 1) {
    set_error("cjoint: bad scores arguments"); return GPT_ERR_BAD_DIMS;
  }
  DevMem dx, ds;
  GPT_HIPCHK(dx.upload(Xtest, (size_t)Ntest * h->D));
  GPT_HIPCHK(ds.alloc<double>((size_t)Ntest * h->C));
  const int rc = gpt_cjoint_scores_dev(h, hyper, Lh, dx.as<double>(), Ntest, ds.as<double>(), nullptr);
  if (rc != GPT_OK) return rc;
  GPT_HIPCHK(ds.download(scores_out, (size_t)Ntest * h->C));
  return GPT_OK;
}

// The per-iteration line of the reference's loop (ImageExperiment.jl:258-268): the scores of the
// test rows at hyper stay on the device and go through gpt_class_eval_dev as one sample.
extern "C" int gpt_cjoint_class_eval(gpt_cjoint* h, const double* hyper, int64_t Lh,
                                     const double* Xtest, const int32_t* ytest, int64_t Ntest,
                                     double* prop_missed_out, double* mean_nlp_out, double* avg_out,
                                     double* mean_scores_out, int32_t* prediction_out,
                                     double* nlp_out, double* scores_out) {
  if (!h || !Xtest || !ytest || !prop_missed_out || !mean_nlp_out || !avg_out || Ntest < 1 ||
      Ntest > (1LL << 31) - 1) {
    set_error("cjoint: bad class_eval arguments"); return GPT_ERR_BAD_DIMS;
  }
  const size_t ns = (size_t)Ntest * h->C;
  DevMem dx, dy, ds, dpm, dnl, davg, dms, dpr, dnp;
  GPT_HIPCHK(dx.upload(Xtest, (size_t)Ntest * h->D));
  GPT_HIPCHK(dy.upload(ytest, (size_t)Ntest));
  GPT_HIPCHK(ds.alloc<double>(ns));
  GPT_HIPCHK(dpm.alloc<double>(1));
  GPT_HIPCHK(dnl.alloc<double>(1));
  GPT_HIPCHK(davg.alloc<double>(2));
  GPT_HIPCHK(dms.alloc<double>(ns));
  GPT_HIPCHK(dpr.alloc<int32_t>((size_t)Ntest));
  GPT_HIPCHK(dnp.alloc<double>((size_t)Ntest));
  int rc = gpt_cjoint_scores_dev(h, hyper, Lh, dx.as<double>(), Ntest, ds.as<double>(), nullptr);
  if (rc != GPT_OK) return rc;
  rc = gpt_class_eval_dev(ds.as<double>(), dy.as<int32_t>(), Ntest, h->C, 1, 0, 1, dpm.as<double>(),
                          dnl.as<double>(), davg.as<double>(), dms.as<double>(), dpr.as<int32_t>(),
                          dnp.as<double>(), nullptr);
  if (rc != GPT_OK) return rc;
  GPT_HIPCHK(dpm.download(prop_missed_out, 1));
  GPT_HIPCHK(dnl.download(mean_nlp_out, 1));
  GPT_HIPCHK(davg.download(avg_out, 2));
  if (mean_scores_out) GPT_HIPCHK(dms.download(mean_scores_out, ns));
  if (prediction_out) GPT_HIPCHK(dpr.download(prediction_out, (size_t)Ntest));
  if (nlp_out) GPT_HIPCHK(dnp.download(nlp_out, (size_t)Ntest));
  if (scores_out) GPT_HIPCHK(ds.download(scores_out, ns));
  return GPT_OK;
}

// Diagnostics (scripts/time_cjoint.py): the device-event time in ms of `reps` back-to-back
// launches of the evaluation in `mode` (0 value, 1 value and d/dtheta, 2 the full gradient, 4 the
// tile's phi and S alone), each with its finish kernel where it has one, divided by reps.
extern "C" int gpt_cjoint_time(gpt_cjoint* h, const double* hyper, int64_t Lh, int32_t mode,
                               int32_t reps, double* ms_out) {
  if (!h || !ms_out || reps < 1 || (mode != kCjValue && mode != kCjTheta && mode != kCjFull &&
                                    mode != kCjFeatures)) {
    set_error("cjoint: bad timing arguments"); return GPT_ERR_BAD_DIMS;
  }
  if (!cj_hyper_ok(hyper, Lh, h->D)) return GPT_ERR_BAD_DIMS;
  hipStream_t st = nullptr;
  CjArgs A;
  double sigma = 0.0;
  const int rc = cj_args(h, hyper, Lh, st, &A, &sigma);
  if (rc != GPT_OK) return rc;
  ScopedEvents ev;
  GPT_HIPCHK(ev.create(2));
  GPT_HIPCHK(hipEventRecord(ev.e[0], st));
  for (int r = 0; r < reps; ++r) {
    GPT_HIPCHK(launch_cjoint_eval(A, h->L, mode, st));
    if (mode == kCjValue || mode == kCjFull)
      GPT_HIPCHK(launch_cjoint_finish(A, h->L, sigma, mode == kCjFull, h->out, st));
  }
  GPT_HIPCHK(hipEventRecord(ev.e[1], st));
  GPT_HIPCHK(hipEventSynchronize(ev.e[1]));
  float ms = 0.f;
  GPT_HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  *ms_out = (double)ms / reps;
  return GPT_OK;
}

// One-shot host-pointer forms (create, body on the fresh handle, destroy).
template <class Body>
static int cj_one_shot(const double* X, int64_t N, int64_t D, const double* y, int64_t C,
                       const double* Z, const double* b, int64_t n, Body&& body) {
  return one_shot<gpt_cjoint>(
      [&](gpt_cjoint** h) { return gpt_cjoint_create(X, N, D, y, C, Z, b, n, h); }, body);
}

// grad_out = [vec(grad theta); grad length_scale; grad sigma_RBF], n*C + Lh entries, the
// reference's layout.
extern "C" int gpt_gpnt_neglogjoint(const double* X, int64_t N, int64_t D, const double* y,
                                    int64_t C, const double* Z, const double* b, int64_t n,
                                    const double* theta, const double* hyper, int64_t Lh,
                                    int64_t want_grad, double* value_out, double* grad_out) {
  if (!cj_dims_ok(X, N, D, C, Z, b, n) || !cj_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  if (!theta || !value_out || (want_grad && !grad_out)) {
    set_error("cjoint: null theta or output"); return GPT_ERR_BAD_DIMS;
  }
  return cj_one_shot(X, N, D, y, C, Z, b, n, [&](gpt_cjoint* h) {
    return gpt_cjoint_eval(h, hyper, Lh, theta, want_grad ? 1 : 0, value_out, grad_out,
                           want_grad ? grad_out + n * C : nullptr);
  });
}

extern "C" int gpt_gpnt_joint_langevin(const double* X, int64_t N, int64_t D, const double* y,
                                       int64_t C, const double* Z, const double* b, int64_t n,
                                       double* theta, const double* hyper, int64_t Lh, double eps,
                                       int64_t nsteps, uint64_t seed, int64_t t0) {
  if (!cj_dims_ok(X, N, D, C, Z, b, n) || !cj_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  if (!theta || t0 < 0) { set_error("cjoint: null theta or negative t0"); return GPT_ERR_BAD_DIMS; }
  return cj_one_shot(X, N, D, y, C, Z, b, n, [&](gpt_cjoint* h) {
    GPT_TRY(gpt_cjoint_set_theta(h, theta));
    GPT_TRY(gpt_cjoint_langevin(h, hyper, Lh, eps, nsteps, seed, t0));
    return gpt_cjoint_get_theta(h, theta);
  });
}

extern "C" int gpt_gpnt_joint_hmc(const double* X, int64_t N, int64_t D, const double* y, int64_t C,
                                  const double* Z, const double* b, int64_t n, double* theta,
                                  const double* hyper, int64_t Lh, double eps, int64_t L,
                                  int64_t burnin, int64_t nsamples, int64_t thin, uint64_t seed,
                                  int64_t t0, double* theta_store, int32_t* accept_out,
                                  double* dH_out, double* value_out, int32_t* ndivergent_out) {
  if (!cj_dims_ok(X, N, D, C, Z, b, n) || !cj_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  if (!theta || t0 < 0) { set_error("cjoint: null theta or negative t0"); return GPT_ERR_BAD_DIMS; }
  return cj_one_shot(X, N, D, y, C, Z, b, n, [&](gpt_cjoint* h) {
    int64_t ndiv = 0;
    GPT_TRY(gpt_cjoint_set_theta(h, theta));
    GPT_TRY(gpt_chmc_run(h, hyper, Lh, eps, L, burnin, nsamples, thin, seed, t0, theta_store,
                         accept_out, dH_out, value_out, &ndiv));
    if (ndivergent_out) *ndivergent_out = (int32_t)ndiv;                 // at most 2^25 transitions
    return gpt_cjoint_get_theta(h, theta);
  });
}

// scores (Ntest, C) = featureNotensor(Xtest)'theta at hyper: no training data is needed.
extern "C" int gpt_gpnt_joint_scores(const double* Xtest, int64_t Ntest, int64_t D, int64_t C,
                                     const double* Z, const double* b, int64_t n,
                                     const double* theta, const double* hyper, int64_t Lh,
                                     double* scores_out) {
  if (!cj_dims_ok(Xtest, Ntest, D, C, Z, b, n) || !cj_hyper_ok(hyper, Lh, D)) return GPT_ERR_BAD_DIMS;
  if (!theta || !scores_out) { set_error("cjoint: null theta or output"); return GPT_ERR_BAD_DIMS; }
  const std::vector<double> ones((size_t)Ntest, 1.0);          // labels are not read by the scores
  return cj_one_shot(Xtest, Ntest, D, ones.data(), C, Z, b, n, [&](gpt_cjoint* h) {
    GPT_TRY(gpt_cjoint_set_theta(h, theta));
    return gpt_cjoint_scores(h, hyper, Lh, Xtest, Ntest, scores_out);
  });
}
