// MovieLens tensor CF from host arrays (100k_movielensExperiment.jl): the SGD / SGLD runs of the
// GPT_*w* variants over folds, and the Gibbs samplers.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_util.h"

using namespace gpt;

// Non-cumulative epoch permutation randperm(N) on the PERM stream of `epoch` (the shuffles of
// 100k_movielensExperiment.jl:451-452 permute the original ratings every epoch).
static void host_randperm(int N, uint64_t seed, int epoch, int32_t* p) {
  for (int i = 0; i < N; ++i) p[i] = i;
  for (int i = N - 1; i >= 1; --i) {
    const uint32_t x = philox4x32((uint32_t)i, (uint32_t)epoch, kPerm, 0, seed).x;
    const int j = (int)(((uint64_t)x * (uint64_t)(i + 1)) >> 32);
    std::swap(p[i], p[j]);
  }
}

static void cf_features(const double* X, int n, int D, int rowbase, std::vector<int32_t>& ptr,
                        std::vector<int32_t>& fe) {
  ptr.assign((size_t)n + 1, 0);
  fe.clear();
  for (int i = 0; i < n; ++i) {
    for (int f = 0; f < D; ++f)
      if (X[i + (size_t)n * f] != 0.0) fe.push_back(rowbase + f);   // find(Data[i,:]) (:430-437)
    ptr[i + 1] = (int32_t)fe.size();
  }
  if (fe.empty()) fe.push_back(0);
}

// 0-based user / movie ids and the ratings of a (count × 3, leading dimension ld) rating array;
// false with the error set when an id is outside the n1 users / n2 movies.
static bool cf_split_ratings(const double* R, int64_t count, int64_t ld, int64_t n1, int64_t n2,
                             const char* what, std::vector<int32_t>& user,
                             std::vector<int32_t>& movie, std::vector<double>& rating) {
  user.resize(count); movie.resize(count); rating.resize(count);
  for (int64_t i = 0; i < count; ++i) {
    user[i] = (int32_t)R[i] - 1; movie[i] = (int32_t)R[i + ld] - 1; rating[i] = R[i + 2 * ld];
    if (user[i] < 0 || user[i] >= n1 || movie[i] < 0 || movie[i] >= n2) { set_error(what); return false; }
  }
  return true;
}

// U, V initialisation of the SGD / SGLD CF samplers (the reference's variants differ):
//   kCfInitSide  GPT_fullw_sideinfo :424-428  stiefel ? polar(randn(r,rows)) : σ_u·randn(rows,r)
//   kCfInitSigma GPT_fixw / GPT_fixw_sideinfo :67 / :294  σ_u·randn(rows,r) (also when stiefel)
//   kCfInitUnit  GPT_fullw :175-180           stiefel ? polar(randn(r,rows)) : randn(rows,r)
enum CfInit { kCfInitSide = 0, kCfInitSigma = 1, kCfInitUnit = 2 };

// One fold's ratings and outputs of a CF run (column-major, caller-owned).
struct CfFold {
  const double* Rating; int64_t N, ldr;
  const double* Ratingtest; int64_t Ntest, ldt;
  double ymean, ystd;
  double *w_store, *U_store, *V_store, *testpred_store, *trainRMSE, *testRMSE;
  int32_t status;                  // out: GPT_OK or GPT_ERR_NAN_GEODESIC
};

// SGD / SGLD runs of the tensor CF model (the body of every GPT_*w* SGD variant) for F folds at
// once: the folds are sibling chains of one cf_epoch_kernel launch per epoch (the reference runs
// them as `@parallel for i=1:5`, 100k_movielensExperiment.jl:733-736), each with its own ratings,
// permutation, state, evaluation and early stop (:541-547); a fold that stops or bails out is
// skipped by later launches.  The folds share the side information, hyper-parameters and seed,
// hence the initial U, V (as separate calls with one param_seed do) and the per-epoch
// permutation; every fold has the same number of training ratings.  fixw keeps w at w_init
// (w_store may then be null); D1 = D2 = 0 with a = 1, b = c = 0 is the model without side
// information.
// Device time of the last CF SGD run on this thread (gpt_cf_last_timing): hipEvents around each
// epoch / eval launch, read after the per-epoch status copy that synchronises anyway.
struct CfTiming { double epoch_ms, eval_ms; int64_t epochs, evals, fold_steps; };
static thread_local CfTiming g_cf_timing{};
static thread_local int32_t g_cf_mode = 0;      // gpt_cf_last_mode
// GPTSGLD_CF_STAMPS=1: per-phase s_memtime of fold 0's first epoch (gpt_cf_last_stamps)
static thread_local std::vector<long long> g_cf_stamps;

// gpt_debug_cf_init's one-shot initial state of the next CF SGD run on this thread
struct CfInject { bool armed = false; int64_t rowsU = 0, rowsV = 0, r = 0; std::vector<double> U, V; };
static thread_local CfInject g_cf_inject;

static int cf_sgd_run(
    const char* name, std::vector<CfFold>& folds, const double* UserData, int64_t n1, int64_t D1,
    const double* MovieData, int64_t n2, int64_t D2, double signal_var, double sigma_u,
    double sigma_w, const double* w_init, int64_t r, int64_t m, double epsw, double epsU, double a,
    double b, double c, int64_t burnin, int64_t maxepoch, uint64_t seed, int32_t langevin,
    int32_t stiefel, int32_t avg, bool fixw, CfInit init) {
  const int F = (int)folds.size();
  CfInject inj;                                      // taken here: cleared however the run ends
  std::swap(inj, g_cf_inject);
  bool ok = F >= 1 && (D1 == 0 || UserData) && (D2 == 0 || MovieData) && w_init && n1 >= 1 &&
            n2 >= 1 && D1 >= 0 && D2 >= 0 && m >= 1 && burnin >= 0 && maxepoch >= 0 &&
            signal_var > 0 && sigma_u > 0 && sigma_w > 0;
  for (const CfFold& f : folds)
    ok = ok && f.Rating && f.Ratingtest && (fixw || f.w_store) && f.U_store && f.V_store &&
         f.testpred_store && f.trainRMSE && f.testRMSE && f.N >= 1 && f.Ntest >= 1 &&
         f.ldr >= f.N && f.ldt >= f.Ntest && f.N == folds[0].N;
  if (!ok) { set_error(std::string("bad ") + name + " arguments"); return GPT_ERR_BAD_DIMS; }
  if (!rank_supported((int)r) || cf_lds_bytes((int)r, (int)m, (int)(D1 + D2), D1 <= 64 && D2 <= 64) > kMaxLds) {
    set_error(std::string(name) + ": rank not instantiated (" + ranks_text() + ") or minibatch too large");
    return GPT_ERR_BAD_DIMS;
  }
  const int64_t N = folds[0].N;
  const int rowsU = (int)(n1 + D1), rowsV = (int)(n2 + D2);
  std::vector<int32_t> uptr, ufe, vptr, vfe;
  cf_features(UserData, (int)n1, (int)D1, (int)n1, uptr, ufe);
  cf_features(MovieData, (int)n2, (int)D2, (int)n2, vptr, vfe);
  // U, V init (:424-428 / :67 / :175-180, see CfInit)
  std::vector<double> U0((size_t)rowsU * r), V0((size_t)rowsV * r);
  for (int which = 0; which < 2; ++which) {
    const int rows = which ? rowsV : rowsU;
    double* M = which ? V0.data() : U0.data();
    std::vector<double> Z((size_t)rows * r);
    for (size_t e = 0; e < Z.size(); ++e) Z[e] = host_normal(seed, (uint32_t)e, 0, kCfUVInit, (uint32_t)which);
    if (stiefel && init != kCfInitSigma) host_stiefel_polar(Z.data(), (int)r, rows, M);
    else if (init == kCfInitUnit) for (size_t e = 0; e < Z.size(); ++e) M[e] = Z[e];
    else for (size_t e = 0; e < Z.size(); ++e) M[e] = sigma_u * Z[e];
  }
  if (inj.armed) {
    if (inj.rowsU != rowsU || inj.rowsV != rowsV || inj.r != r) {
      set_error(std::string(name) + ": the injected U0 / V0 (gpt_debug_cf_init) are " +
                std::to_string(inj.rowsU) + " and " + std::to_string(inj.rowsV) + " rows of rank " +
                std::to_string(inj.r) + ", the run has " + std::to_string(rowsU) + " and " +
                std::to_string(rowsV) + " of rank " + std::to_string(r));
      return GPT_ERR_BAD_DIMS;
    }
    U0 = inj.U; V0 = inj.V;
  }
  const size_t nU = U0.size(), nV = V0.size(), rr = (size_t)r * r;
  const int nbatch = (int)((N + m - 1) / m);
  int64_t ntmax = 0;
  for (const CfFold& f : folds) ntmax = std::max(ntmax, f.Ntest);
  const int nmax = (int)std::max(N, ntmax);
  const int neval = (nmax + 255) / 256;
  DevMem d_up, d_uf, d_vp, d_vf, d_perm, d_ch;
  GPT_HIPCHK(d_up.upload(uptr.data(), uptr.size()));
  GPT_HIPCHK(d_uf.upload(ufe.data(), ufe.size()));
  GPT_HIPCHK(d_vp.upload(vptr.data(), vptr.size()));
  GPT_HIPCHK(d_vf.upload(vfe.data(), vfe.size()));
  GPT_HIPCHK(d_perm.alloc<int32_t>(N));
  // per fold: ratings, state, scratch, running predictions, SSE partials, status
  DevSet mem;
  std::vector<CfChain> ch(F);
  std::vector<int32_t*> d_st(F);
  std::vector<double*> d_w(F), d_U(F), d_V(F), d_sse(F), d_tep(F);
  std::vector<int32_t> tu, tm, eu, em;
  std::vector<double> tr, er;
  for (int f = 0; f < F; ++f) {
    const CfFold& fd = folds[f];
    const int64_t Nt = fd.Ntest;
    if (!cf_split_ratings(fd.Rating, N, fd.ldr, n1, n2, "rating ids out of range", tu, tm, tr) ||
        !cf_split_ratings(fd.Ratingtest, Nt, fd.ldt, n1, n2, "test rating ids out of range", eu, em, er))
      return GPT_ERR_BAD_DIMS;
    // one allocation per fold: ids (int32) first, then doubles (8-B aligned offsets)
    const size_t ints = (size_t)(4 * N + 2 * Nt + 2);
    const size_t dbl0 = (ints * 4 + 15) / 16 * 2;                     // in doubles
    const size_t ndbl = (size_t)N + Nt + rr + 2 * nU + 2 * nV + N + Nt + 2 * (size_t)neval + N;
    double* blk = nullptr;
    GPT_HIPCHK(mem.alloc(&blk, dbl0 + ndbl));
    int32_t* ip = (int32_t*)blk;
    double* dp = blk + dbl0;
    CfChain& C = ch[f];
    C.tr_user = ip; C.tr_movie = ip + N; C.te_user = ip + 2 * N; C.te_movie = ip + 2 * N + Nt;
    d_st[f] = ip + 2 * N + 2 * Nt;
    C.tr_rating = dp; C.te_rating = dp + N;
    C.w = dp + N + Nt; C.U = C.w + rr; C.V = C.U + nU; C.GU = C.V + nV; C.GV = C.GU + nU;
    C.trainpred = C.GV + nV; C.testpred = C.trainpred + N; C.sse = C.testpred + Nt;
    C.ep_user = ip + 2 * N + 2 * Nt + 2; C.ep_movie = C.ep_user + N;
    C.ep_rating = C.sse + 2 * (size_t)neval;
    C.N = (int)N; C.Ntest = (int)Nt; C.perm = d_perm.as<int32_t>();
    C.status = d_st[f]; C.ymean = fd.ymean; C.ystd = fd.ystd;
    d_w[f] = C.w; d_U[f] = C.U; d_V[f] = C.V; d_sse[f] = C.sse; d_tep[f] = C.testpred;
    GPT_HIPCHK(hipMemcpy((void*)C.tr_user, tu.data(), 4 * N, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemcpy((void*)C.tr_movie, tm.data(), 4 * N, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemcpy((void*)C.te_user, eu.data(), 4 * Nt, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemcpy((void*)C.te_movie, em.data(), 4 * Nt, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemcpy((void*)C.tr_rating, tr.data(), 8 * N, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemcpy((void*)C.te_rating, er.data(), 8 * Nt, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemcpy(C.w, w_init, 8 * rr, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemcpy(C.U, U0.data(), 8 * nU, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemcpy(C.V, V0.data(), 8 * nV, hipMemcpyHostToDevice));
    GPT_HIPCHK(hipMemset(C.GU, 0, 8 * (nU + nV)));                             // GU, GV
    GPT_HIPCHK(hipMemset(C.trainpred, 0, 8 * (size_t)(N + Nt)));
    GPT_HIPCHK(hipMemset(d_st[f], 0, 4));
  }
  GPT_HIPCHK(d_ch.upload(ch.data(), ch.size()));
  CfParams P{};
  P.n1 = (int)n1; P.D1 = (int)D1; P.n2 = (int)n2; P.D2 = (int)D2; P.r = (int)r; P.m = (int)m;
  P.rowsU = rowsU; P.rowsV = rowsV;
  P.a = a; P.b = b; P.c = c; P.signal_var = signal_var; P.sigma_u = sigma_u; P.sigma_w = sigma_w;
  P.epsw = epsw; P.epsU = epsU; P.langevin = langevin; P.stiefel = stiefel; P.seed = seed;
  P.fixw = fixw ? 1 : 0;
  P.uptr = d_up.as<int32_t>(); P.ufe = d_uf.as<int32_t>(); P.vptr = d_vp.as<int32_t>(); P.vfe = d_vf.as<int32_t>();
  DevMem d_masks;
  if (D1 <= 64 && D2 <= 64) {    // each user's / movie's feature rows as one 64-bit mask
    std::vector<uint64_t> mk((size_t)(n1 + n2), 0);
    for (int64_t i = 0; i < n1; ++i)
      for (int z = uptr[i]; z < uptr[i + 1]; ++z) mk[i] |= 1ull << (ufe[z] - n1);
    for (int64_t i = 0; i < n2; ++i)
      for (int z = vptr[i]; z < vptr[i + 1]; ++z) mk[n1 + i] |= 1ull << (vfe[z] - n2);
    GPT_HIPCHK(d_masks.upload(mk.data(), mk.size()));
    P.umask = d_masks.as<uint64_t>();
    P.vmask = P.umask + n1;
  }
  DevMem d_stamps;
  const bool want_stamps = std::getenv("GPTSGLD_CF_STAMPS") != nullptr;
  g_cf_stamps.clear();
  if (want_stamps) {
    GPT_HIPCHK(d_stamps.alloc<long long>((size_t)kCfStampSteps * kCfStampSlots));
    GPT_HIPCHK(d_stamps.zero());
    P.stamps = d_stamps.as<long long>();
  }
#if CF_WSTAMPS
  if (std::getenv("GPTSGLD_CF_EXP")) P.exp = std::atoi(std::getenv("GPTSGLD_CF_EXP"));
#endif
  for (CfFold& fd : folds) {
    if (fd.w_store) std::memset(fd.w_store, 0, 8 * rr * maxepoch);
    std::memset(fd.U_store, 0, 8 * nU * maxepoch);
    std::memset(fd.V_store, 0, 8 * nV * maxepoch);
    std::memset(fd.testpred_store, 0, 8 * (size_t)fd.Ntest * maxepoch);
    std::memset(fd.trainRMSE, 0, 8 * (size_t)maxepoch);
    for (int64_t z = 0; z < maxepoch; ++z) fd.testRMSE[z] = 10.0;            // :441
    fd.status = GPT_OK;
  }
  std::vector<int32_t> perm(N);
  std::vector<double> sse(2 * (size_t)neval), tp(ntmax);
  std::vector<char> live(F, 1);
  std::vector<int> testcounter(F, 0);
  int counter = 0, nlive = F;
  long long step_base_host = 0;                      // graph replays' epoch base: read by the copy
                                                     // below, alive until the epoch's event sync
  const int32_t stopped = 2;                         // skips the fold in later launches
  ScopedEvents evs;
  GPT_HIPCHK(evs.create(4));
  // the run's own stream; the SGD / SGLD path replays one captured graph per epoch (gather + the
  // epoch's batch-phase / move launch pairs), its steps counted from a device-side epoch base
  struct RunStream {
    hipStream_t s = nullptr;
    hipGraph_t g = nullptr;
    hipGraphExec_t x = nullptr;
    ~RunStream() {
      if (s) (void)hipStreamSynchronize(s);
      if (x) (void)hipGraphExecDestroy(x);
      if (g) (void)hipGraphDestroy(g);
      if (s) (void)hipStreamDestroy(s);
    }
  } rs;
  GPT_HIPCHK(hipStreamCreateWithFlags(&rs.s, hipStreamNonBlocking));
  hipStream_t st = rs.s;
  GPT_HIPCHK(hipStreamSynchronize(nullptr));         // the set-up copies / memsets are done
  DevMem d_step;
  GPT_HIPCHK(d_step.alloc<long long>(1));
  g_cf_timing = CfTiming{};
  // SGD (no Langevin noise, no Stiefel geometry) on the feature-mask path: the lazy move, one
  // launch per epoch (cf_epoch_kernel domove = 2); GPTSGLD_CF_LAZY=0 keeps the batch-phase / move
  // launch pairs
  // (the decay factor c = 1 − εU/(2σ_u²) of a skipped row must lie in (0, 1): the kernel reads a
  // row Δ steps behind as m·c^Δ; outside that range the eager move keeps the reference's numbers)
  const double cdecay = 1.0 - P.epsU / (2.0 * P.sigma_u * P.sigma_u);
  const bool lazy = !stiefel && !langevin && P.umask != nullptr && cdecay > 0.0 && cdecay < 1.0 &&
                    cf_lazy_lds_bytes((int)r, (int)m, (int)(D1 + D2), rowsU + rowsV, nbatch) <=
                        kMaxLds &&
                    !(std::getenv("GPTSGLD_CF_LAZY") && std::strcmp(std::getenv("GPTSGLD_CF_LAZY"), "0") == 0);
  g_cf_mode = stiefel ? 1 : (lazy ? 2 : 0);
  for (int64_t epoch = 1; epoch <= burnin + maxepoch && nlive > 0; ++epoch) {
    host_randperm((int)N, seed, (int)(epoch - 1), perm.data());
    GPT_HIPCHK(hipMemcpy(d_perm.p, perm.data(), d_perm.bytes, hipMemcpyHostToDevice));
    hipError_t e = hipSuccess;
    if (stiefel || lazy) {
      // the Stiefel move needs Grams over every row, the lazy SGD move needs none of the rows
      // outside the batch: the whole epoch in one workgroup per fold, one launch
      GPT_HIPCHK(hipEventRecord(evs.e[0], st));
      e = launch_cf_gather(d_ch.as<CfChain>(), F, (int)N, st);
      if (e == hipSuccess)
        e = launch_cf_epoch(P, d_ch.as<CfChain>(), F, (epoch - 1) * nbatch, 0, nbatch,
                            stiefel ? 1 : 2, st);
    } else if (P.stamps) {
      // the stamped first epoch: direct launches (the stamp buffer is dropped after it)
      GPT_HIPCHK(hipEventRecord(evs.e[0], st));
      e = launch_cf_gather(d_ch.as<CfChain>(), F, (int)N, st);
      for (int b = 0; b < nbatch && e == hipSuccess; ++b) {
        const long long step = (epoch - 1) * nbatch + b;
        e = launch_cf_epoch(P, d_ch.as<CfChain>(), F, step, b, 1, 0, st);
        if (e == hipSuccess) e = launch_cf_move(P, d_ch.as<CfChain>(), F, step, st);
      }
    } else {
      // per minibatch: the batch phase (one workgroup per fold), then the row-parallel move of U
      // and V over the whole GPU (cf_move_kernel) — an epoch of them as one graph
      if (!rs.x) {
        GPT_HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        e = launch_cf_gather(d_ch.as<CfChain>(), F, (int)N, st);
        for (int b = 0; b < nbatch && e == hipSuccess; ++b) {
          e = launch_cf_epoch(P, d_ch.as<CfChain>(), F, b, b, 1, 0, st, d_step.as<long long>());
          if (e == hipSuccess)
            e = launch_cf_move(P, d_ch.as<CfChain>(), F, b, st, d_step.as<long long>());
        }
        const hipError_t ec = hipStreamEndCapture(st, &rs.g);
        if (e != hipSuccess) return hip_fail(e, "cf epoch capture");
        if (ec != hipSuccess) return hip_fail(ec, "hipStreamEndCapture");
        GPT_HIPCHK(hipGraphInstantiate(&rs.x, rs.g, nullptr, nullptr, 0));
      }
      step_base_host = (epoch - 1) * nbatch;
      GPT_HIPCHK(hipMemcpyAsync(d_step.p, &step_base_host, sizeof(long long), hipMemcpyHostToDevice, st));
      GPT_HIPCHK(hipEventRecord(evs.e[0], st));
      e = hipGraphLaunch(rs.x, st);
    }
    if (e != hipSuccess) return hip_fail(e, "cf epoch kernel");
    GPT_HIPCHK(hipEventRecord(evs.e[1], st));
    GPT_HIPCHK(hipEventSynchronize(evs.e[1]));
    if (P.stamps) {                // the first epoch only
      g_cf_stamps.resize((size_t)kCfStampSteps * kCfStampSlots);
      GPT_HIPCHK(d_stamps.download(g_cf_stamps.data(), g_cf_stamps.size()));
      P.stamps = nullptr;
    }
    {
      float ms = 0.f;
      GPT_HIPCHK(hipEventElapsedTime(&ms, evs.e[0], evs.e[1]));
      g_cf_timing.epoch_ms += ms;
      g_cf_timing.epochs += 1;
      g_cf_timing.fold_steps += (int64_t)nlive * nbatch;
    }
    for (int f = 0; f < F; ++f) {
      if (!live[f]) continue;
      int32_t bad = 0;
      GPT_HIPCHK(hipMemcpy(&bad, d_st[f], 4, hipMemcpyDeviceToHost));
      if (bad) {                     // :490-492 — zero parameter stores, curves as they are
        CfFold& fd = folds[f];
        if (fd.w_store) std::memset(fd.w_store, 0, 8 * rr * maxepoch);
        std::memset(fd.U_store, 0, 8 * nU * maxepoch);
        std::memset(fd.V_store, 0, 8 * nV * maxepoch);
        fd.status = GPT_ERR_NAN_GEODESIC;
        live[f] = 0; --nlive;
      }
    }
    if (epoch > burnin && nlive > 0) {
      const int64_t s2 = epoch - burnin - 1;
      if (!avg) counter = 0;
      GPT_HIPCHK(hipEventRecord(evs.e[2], st));
      e = launch_cf_eval(P, d_ch.as<CfChain>(), F, nmax, counter, st);
      if (e != hipSuccess) return hip_fail(e, "cf eval kernel");
      GPT_HIPCHK(hipEventRecord(evs.e[3], st));
      GPT_HIPCHK(hipEventSynchronize(evs.e[3]));
      {
        float ms = 0.f;
        GPT_HIPCHK(hipEventElapsedTime(&ms, evs.e[2], evs.e[3]));
        g_cf_timing.eval_ms += ms;
        g_cf_timing.evals += 1;
      }
      for (int f = 0; f < F; ++f) {
        if (!live[f]) continue;
        CfFold& fd = folds[f];
        if (fd.w_store) GPT_HIPCHK(hipMemcpy(fd.w_store + rr * s2, d_w[f], 8 * rr, hipMemcpyDeviceToHost));
        GPT_HIPCHK(hipMemcpy(fd.U_store + nU * s2, d_U[f], 8 * nU, hipMemcpyDeviceToHost));
        GPT_HIPCHK(hipMemcpy(fd.V_store + nV * s2, d_V[f], 8 * nV, hipMemcpyDeviceToHost));
        GPT_HIPCHK(hipMemcpy(sse.data(), d_sse[f], 16 * (size_t)neval, hipMemcpyDeviceToHost));
        GPT_HIPCHK(hipMemcpy(tp.data(), d_tep[f], 8 * fd.Ntest, hipMemcpyDeviceToHost));
        double st0 = 0.0, st1 = 0.0;
        for (int z = 0; z < neval; ++z) { st0 += sse[2 * z]; st1 += sse[2 * z + 1]; }
        fd.trainRMSE[s2] = std::sqrt(st0 / (double)N);
        fd.testRMSE[s2] = std::sqrt(st1 / (double)fd.Ntest);
        for (int64_t i = 0; i < fd.Ntest; ++i)
          fd.testpred_store[(size_t)fd.Ntest * s2 + i] =
              std::min(std::max(tp[i] * fd.ystd + fd.ymean, 1.0), 5.0);
        // :541-547 (the reference compares with the previous epoch's entry; none at s2 = 0)
        if (epoch > 1 && s2 > 0 && fd.testRMSE[s2] > fd.testRMSE[s2 - 1]) testcounter[f] += 1;
        else testcounter[f] = 0;
        if (testcounter[f] >= 5) {
          GPT_HIPCHK(hipMemcpy(d_st[f], &stopped, 4, hipMemcpyHostToDevice));
          live[f] = 0; --nlive;
        }
      }
      counter += 1;
    }
  }
  for (const CfFold& fd : folds)
    if (fd.status != GPT_OK) {
      set_error("Get NaN when moving along Geodesic. Try smaller epsU");
      return GPT_ERR_NAN_GEODESIC;
    }
  return GPT_OK;
}

// one fold (the reference functions' own signature)
static int cf_sgd_one(const char* name, const double* Rating, int64_t N, int64_t ldr,
                      const double* UserData, int64_t n1, int64_t D1, const double* MovieData,
                      int64_t n2, int64_t D2, const double* Ratingtest, int64_t Ntest, int64_t ldt,
                      double signal_var, double sigma_u, double sigma_w, const double* w_init,
                      int64_t r, int64_t m, double epsw, double epsU, double a, double b, double c,
                      int64_t burnin, int64_t maxepoch, uint64_t seed, double ytrainMean,
                      double ytrainStd, int32_t langevin, int32_t stiefel, int32_t avg, bool fixw,
                      CfInit init, double* w_store, double* U_store, double* V_store,
                      double* testpred_store, double* trainRMSE, double* testRMSE) {
  std::vector<CfFold> folds(1);
  folds[0] = CfFold{Rating, N, ldr, Ratingtest, Ntest, ldt, ytrainMean, ytrainStd, w_store, U_store,
                    V_store, testpred_store, trainRMSE, testRMSE, GPT_OK};
  return cf_sgd_run(name, folds, UserData, n1, D1, MovieData, n2, D2, signal_var, sigma_u, sigma_w,
                    w_init, r, m, epsw, epsU, a, b, c, burnin, maxepoch, seed, langevin, stiefel,
                    avg, fixw, init);
}

extern "C" int gpt_cf_fullw_sideinfo(
    const double* Rating, int64_t N, int64_t ldr, const double* UserData, int64_t n1, int64_t D1,
    const double* MovieData, int64_t n2, int64_t D2, const double* Ratingtest, int64_t Ntest,
    int64_t ldt, double signal_var, double sigma_u, double sigma_w, const double* w_init, int64_t r,
    int64_t m, double epsw, double epsU, double a, double b, double c, int64_t burnin,
    int64_t maxepoch, uint64_t seed, double ytrainMean, double ytrainStd, int32_t langevin,
    int32_t stiefel, int32_t avg, double* w_store, double* U_store, double* V_store,
    double* testpred_store, double* trainRMSE, double* testRMSE) {
  return cf_sgd_one("GPT_fullw_sideinfo", Rating, N, ldr, UserData, n1, D1, MovieData, n2, D2,
                    Ratingtest, Ntest, ldt, signal_var, sigma_u, sigma_w, w_init, r, m, epsw, epsU,
                    a, b, c, burnin, maxepoch, seed, ytrainMean, ytrainStd, langevin, stiefel, avg,
                    false, kCfInitSide, w_store, U_store, V_store, testpred_store, trainRMSE,
                    testRMSE);
}

extern "C" int gpt_cf_fullw_sideinfo_folds(
    int64_t F, const double* const* Rating, const int64_t* N, const double* const* Ratingtest,
    const int64_t* Ntest, const double* UserData, int64_t n1, int64_t D1, const double* MovieData,
    int64_t n2, int64_t D2, double signal_var, double sigma_u, double sigma_w,
    const double* w_init, int64_t r, int64_t m, double epsw, double epsU, double a, double b,
    double c, int64_t burnin, int64_t maxepoch, uint64_t seed, const double* ytrainMean,
    const double* ytrainStd, int32_t langevin, int32_t stiefel, int32_t avg,
    double* const* w_store, double* const* U_store, double* const* V_store,
    double* const* testpred_store, double* const* trainRMSE, double* const* testRMSE,
    int32_t* status) {
  if (F < 1 || F > 65535 || !Rating || !N || !Ratingtest || !Ntest || !ytrainMean || !ytrainStd ||
      !w_store || !U_store || !V_store || !testpred_store || !trainRMSE || !testRMSE) {
    set_error("bad GPT_fullw_sideinfo_folds arguments"); return GPT_ERR_BAD_DIMS;
  }
  std::vector<CfFold> folds(F);
  for (int64_t f = 0; f < F; ++f)
    folds[f] = CfFold{Rating[f], N[f], N[f], Ratingtest[f], Ntest[f], Ntest[f], ytrainMean[f],
                      ytrainStd[f], w_store[f], U_store[f], V_store[f], testpred_store[f],
                      trainRMSE[f], testRMSE[f], GPT_OK};
  const int rc = cf_sgd_run("GPT_fullw_sideinfo_folds", folds, UserData, n1, D1, MovieData, n2, D2,
                            signal_var, sigma_u, sigma_w, w_init, r, m, epsw, epsU, a, b, c,
                            burnin, maxepoch, seed, langevin, stiefel, avg, false, kCfInitSide);
  if (status)
    for (int64_t f = 0; f < F; ++f) status[f] = folds[f].status;
  return rc;
}

extern "C" int gpt_debug_cf_init(const double* U0, int64_t rowsU, const double* V0, int64_t rowsV,
                                 int64_t r) {
  g_cf_inject = CfInject{};
  if (!U0 && !V0) return GPT_OK;                     // disarm
  if (!U0 || !V0 || rowsU < 1 || rowsV < 1 || r < 1) {
    set_error("gpt_debug_cf_init: U0 and V0 (rows >= 1, r >= 1), or both null");
    return GPT_ERR_BAD_DIMS;
  }
  g_cf_inject.U.assign(U0, U0 + (size_t)rowsU * r);
  g_cf_inject.V.assign(V0, V0 + (size_t)rowsV * r);
  g_cf_inject.rowsU = rowsU; g_cf_inject.rowsV = rowsV; g_cf_inject.r = r;
  g_cf_inject.armed = true;
  return GPT_OK;
}

extern "C" int gpt_cf_last_timing(double* epoch_ms, double* eval_ms, int64_t* epochs,
                                   int64_t* fold_steps) {
  if (!epoch_ms || !eval_ms || !epochs || !fold_steps) {
    set_error("gpt_cf_last_timing: null output"); return GPT_ERR_BAD_DIMS;
  }
  *epoch_ms = g_cf_timing.epoch_ms;
  *eval_ms = g_cf_timing.eval_ms;
  *epochs = g_cf_timing.epochs;
  *fold_steps = g_cf_timing.fold_steps;
  return GPT_OK;
}

extern "C" int gpt_cf_last_mode(int32_t* mode) {
  if (!mode) { set_error("gpt_cf_last_mode: null output"); return GPT_ERR_BAD_DIMS; }
  *mode = g_cf_mode;
  return GPT_OK;
}

extern "C" int64_t gpt_cf_last_stamps(int64_t* out, int64_t cap) {
  const int64_t n = (int64_t)g_cf_stamps.size();
  if (out)
    for (int64_t i = 0; i < std::min(n, cap); ++i) out[i] = g_cf_stamps[(size_t)i];
  return n;
}

extern "C" int gpt_cf_fixw_sideinfo(
    const double* Rating, int64_t N, int64_t ldr, const double* UserData, int64_t n1, int64_t D1,
    const double* MovieData, int64_t n2, int64_t D2, const double* Ratingtest, int64_t Ntest,
    int64_t ldt, double signal_var, double sigma_u, const double* w, int64_t r, int64_t m,
    double epsU, double a, double b, double c, int64_t burnin, int64_t maxepoch, uint64_t seed,
    double ytrainMean, double ytrainStd, int32_t langevin, int32_t stiefel, int32_t avg,
    double* U_store, double* V_store, double* testpred_store, double* trainRMSE,
    double* testRMSE) {
  return cf_sgd_one("GPT_fixw_sideinfo", Rating, N, ldr, UserData, n1, D1, MovieData, n2, D2,
                    Ratingtest, Ntest, ldt, signal_var, sigma_u, 1.0, w, r, m, 0.0, epsU, a, b, c,
                    burnin, maxepoch, seed, ytrainMean, ytrainStd, langevin, stiefel, avg, true,
                    kCfInitSigma, nullptr, U_store, V_store, testpred_store, trainRMSE, testRMSE);
}

extern "C" int gpt_cf_fullw(const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
                            const double* Ratingtest, int64_t Ntest, int64_t ldt,
                            double signal_var, double sigma_u, double sigma_w,
                            const double* w_init, int64_t r, int64_t m, double epsw, double epsU,
                            int64_t burnin, int64_t maxepoch, uint64_t seed, double ytrainMean,
                            double ytrainStd, int32_t langevin, int32_t stiefel, int32_t avg,
                            double* w_store, double* U_store, double* V_store,
                            double* testpred_store, double* trainRMSE, double* testRMSE) {
  return cf_sgd_one("GPT_fullw", Rating, N, ldr, nullptr, n1, 0, nullptr, n2, 0, Ratingtest,
                    Ntest, ldt, signal_var, sigma_u, sigma_w, w_init, r, m, epsw, epsU, 1.0, 0.0,
                    0.0, burnin, maxepoch, seed, ytrainMean, ytrainStd, langevin, stiefel, avg,
                    false, kCfInitUnit, w_store, U_store, V_store, testpred_store, trainRMSE,
                    testRMSE);
}

extern "C" int gpt_cf_fixw(const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
                           const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var,
                           double sigma_u, const double* w, int64_t r, int64_t m, double epsU,
                           int64_t burnin, int64_t maxepoch, uint64_t seed, double ytrainMean,
                           double ytrainStd, int32_t langevin, int32_t stiefel, int32_t avg,
                           double* U_store, double* V_store, double* testpred_store,
                           double* trainRMSE, double* testRMSE) {
  return cf_sgd_one("GPT_fixw", Rating, N, ldr, nullptr, n1, 0, nullptr, n2, 0, Ratingtest, Ntest,
                    ldt, signal_var, sigma_u, 1.0, w, r, m, 0.0, epsU, 1.0, 0.0, 0.0, burnin,
                    maxepoch, seed, ytrainMean, ytrainStd, langevin, stiefel, avg, true,
                    kCfInitSigma, nullptr, U_store, V_store, testpred_store, trainRMSE, testRMSE);
}

// Q of a Householder QR (LAPACK dgeqr2 + dorg2r conventions), r × r column-major in place.
static void host_qr_q(int r, std::vector<double>& A) {
  std::vector<double> tau(r, 0.0);
  for (int k = 0; k < r; ++k) {
    double xn = 0.0;
    for (int i = k + 1; i < r; ++i) xn = std::hypot(xn, A[i + (size_t)r * k]);
    const double alpha = A[k + (size_t)r * k];
    if (xn == 0.0) { tau[k] = 0.0; continue; }
    const double beta = -std::copysign(std::hypot(alpha, xn), alpha);
    tau[k] = (beta - alpha) / beta;
    const double sc = 1.0 / (alpha - beta);
    for (int i = k + 1; i < r; ++i) A[i + (size_t)r * k] *= sc;
    A[k + (size_t)r * k] = beta;
    for (int j = k + 1; j < r; ++j) {            // apply H_k to the trailing columns
      double s = A[k + (size_t)r * j];
      for (int i = k + 1; i < r; ++i) s += A[i + (size_t)r * k] * A[i + (size_t)r * j];
      s *= tau[k];
      A[k + (size_t)r * j] -= s;
      for (int i = k + 1; i < r; ++i) A[i + (size_t)r * j] -= s * A[i + (size_t)r * k];
    }
  }
  std::vector<double> Qm((size_t)r * r, 0.0);
  for (int i = 0; i < r; ++i) Qm[i + (size_t)r * i] = 1.0;
  for (int k = r - 1; k >= 0; --k) {             // Q = H_0 … H_{r-1} applied to I (dorg2r)
    for (int j = k; j < r; ++j) {
      double s = Qm[k + (size_t)r * j];
      for (int i = k + 1; i < r; ++i) s += A[i + (size_t)r * k] * Qm[i + (size_t)r * j];
      s *= tau[k];
      Qm[k + (size_t)r * j] -= s;
      for (int i = k + 1; i < r; ++i) Qm[i + (size_t)r * j] -= s * A[i + (size_t)r * k];
    }
  }
  A.swap(Qm);
}

// Gibbs sweeps of the CF model without side information (GPT_fullw_gibbs; fixw: GPT_fixw_gibbs,
// :945-1028 — the same user / movie conditionals, no w draw, w_store may be null).
static int cf_gibbs_run(
    const char* name, const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
    const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var, double sigma_u,
    double sigma_w, const double* w_init, int64_t r, int64_t burnin, int64_t maxepoch,
    int64_t n_samples, uint64_t seed, double ytrainMean, double ytrainStd, int32_t avg,
    int32_t rotated_w, bool fixw, double* w_store, double* U_store, double* V_store,
    double* testpred_store, double* trainRMSE, double* testRMSE) {
  if (!Rating || !Ratingtest || !w_init || (!fixw && !w_store) || !U_store || !V_store || !testpred_store ||
      !trainRMSE || !testRMSE || N < 1 || Ntest < 1 || ldr < N || ldt < Ntest || n1 < 1 || n2 < 1 ||
      burnin < 0 || maxepoch < 0 || n_samples < 1 || !(signal_var > 0) || !(sigma_u > 0) ||
      !(sigma_w > 0)) {
    set_error(std::string("bad ") + name + " arguments"); return GPT_ERR_BAD_DIMS;
  }
  if (!rank_supported((int)r) || r * r > 1024) {
    set_error(std::string(name) + ": rank not instantiated (" + ranks_text() + ")"); return GPT_ERR_BAD_DIMS;
  }
  std::vector<int32_t> tu, tm, eu, em;
  std::vector<double> tr, er;
  if (!cf_split_ratings(Rating, N, ldr, n1, n2, "rating ids out of range", tu, tm, tr) ||
      !cf_split_ratings(Ratingtest, Ntest, ldt, n1, n2, "test rating ids out of range", eu, em, er))
    return GPT_ERR_BAD_DIMS;
  // ratings of each user / movie in Rating order (idx = (Rating[:,1].==i), :1061)
  std::vector<int32_t> uptr(n1 + 1, 0), mptr(n2 + 1, 0), ulst(N), mlst(N);
  for (int64_t i = 0; i < N; ++i) { uptr[tu[i] + 1]++; mptr[tm[i] + 1]++; }
  for (int64_t i = 0; i < n1; ++i) uptr[i + 1] += uptr[i];
  for (int64_t i = 0; i < n2; ++i) mptr[i + 1] += mptr[i];
  {
    std::vector<int32_t> cu(uptr.begin(), uptr.end() - 1), cm(mptr.begin(), mptr.end() - 1);
    for (int64_t i = 0; i < N; ++i) { ulst[cu[tu[i]]++] = (int32_t)i; mlst[cm[tm[i]]++] = (int32_t)i; }
  }
  // init (:1047-1053): Q = qr(randn(r,r)), U = σ_u·randn(n1,r), V = σ_u·randn(n2,r)
  const size_t rr = (size_t)r * r, nU = (size_t)n1 * r, nV = (size_t)n2 * r;
  std::vector<double> Qm(rr), U0(nU), V0(nV), w0(w_init, w_init + rr);
  for (size_t e = 0; e < rr; ++e) Qm[e] = host_normal(seed, (uint32_t)e, 0, kCfgInit, 0);
  for (size_t e = 0; e < nU; ++e) U0[e] = sigma_u * host_normal(seed, (uint32_t)e, 0, kCfgInit, 1);
  for (size_t e = 0; e < nV; ++e) V0[e] = sigma_u * host_normal(seed, (uint32_t)e, 0, kCfgInit, 2);
  host_qr_q((int)r, Qm);
  if (rotated_w) {                                // w = Q·w_init; U = U·Q'
    for (int64_t i = 0; i < r; ++i)
      for (int64_t j = 0; j < r; ++j) {
        double s = 0.0;
        for (int64_t k = 0; k < r; ++k) s += Qm[i + r * k] * w_init[k + r * j];
        w0[i + r * j] = s;
      }
    std::vector<double> U1(nU);
    for (int64_t i = 0; i < n1; ++i)
      for (int64_t j = 0; j < r; ++j) {
        double s = 0.0;
        for (int64_t k = 0; k < r; ++k) s += U0[i + n1 * k] * Qm[j + r * k];
        U1[i + n1 * j] = s;
      }
    U0.swap(U1);
  }
  const int p = (int)rr;
  const int neval = (int)((std::max(N, Ntest) + 255) / 256);
  DevMem d_tu, d_tm, d_tr, d_eu, d_em, d_er, d_up, d_mp, d_ul, d_ml, d_w, d_U, d_V, d_M, d_x,
      d_z, d_trp, d_tep, d_sse, d_st, d_ch, d_zu, d_zv, d_ws, d_keep;
  GPT_HIPCHK(d_tu.upload(tu.data(), tu.size()));
  GPT_HIPCHK(d_tm.upload(tm.data(), tm.size()));
  GPT_HIPCHK(d_tr.upload(tr.data(), tr.size()));
  GPT_HIPCHK(d_eu.upload(eu.data(), eu.size()));
  GPT_HIPCHK(d_em.upload(em.data(), em.size()));
  GPT_HIPCHK(d_er.upload(er.data(), er.size()));
  GPT_HIPCHK(d_up.upload(uptr.data(), uptr.size()));
  GPT_HIPCHK(d_mp.upload(mptr.data(), mptr.size()));
  GPT_HIPCHK(d_ul.upload(ulst.data(), ulst.size()));
  GPT_HIPCHK(d_ml.upload(mlst.data(), mlst.size()));
  GPT_HIPCHK(d_w.upload(w0.data(), w0.size()));
  GPT_HIPCHK(d_U.upload(U0.data(), U0.size()));
  GPT_HIPCHK(d_V.upload(V0.data(), V0.size()));
  GPT_HIPCHK(d_M.alloc<double>(rr * rr));
  GPT_HIPCHK(d_x.alloc<double>(rr));
  GPT_HIPCHK(d_z.alloc<double>(rr));
  GPT_HIPCHK(d_sse.alloc<double>(2 * (size_t)neval));
  GPT_HIPCHK(d_ws.alloc<double>(cfg_wsystem_scratch_dbl((int)r, (int)n1)));
  GPT_HIPCHK(d_trp.alloc<double>(N));
  GPT_HIPCHK(d_trp.zero());
  GPT_HIPCHK(d_tep.alloc<double>(Ntest));
  GPT_HIPCHK(d_tep.zero());
  GPT_HIPCHK(d_st.alloc<int32_t>(1));
  GPT_HIPCHK(d_st.zero());
  GPT_HIPCHK(d_zu.alloc<int32_t>(n1 + 1));
  GPT_HIPCHK(d_zu.zero());
  GPT_HIPCHK(d_zv.alloc<int32_t>(n2 + 1));
  GPT_HIPCHK(d_zv.zero());
  // prediction without side information: a = 1, b = c = 0, empty feature lists (:1101-1102)
  CfParams P{};
  P.n1 = (int)n1; P.D1 = 0; P.n2 = (int)n2; P.D2 = 0; P.r = (int)r; P.m = 1;
  P.rowsU = (int)n1; P.rowsV = (int)n2; P.a = 1.0; P.b = 0.0; P.c = 0.0;
  P.signal_var = signal_var; P.sigma_u = sigma_u; P.sigma_w = sigma_w; P.seed = seed;
  P.uptr = d_zu.as<int32_t>(); P.ufe = d_zu.as<int32_t>(); P.vptr = d_zv.as<int32_t>(); P.vfe = d_zv.as<int32_t>();
  CfChain Cc{};
  Cc.tr_user = d_tu.as<int32_t>(); Cc.tr_movie = d_tm.as<int32_t>(); Cc.tr_rating = d_tr.as<double>();
  Cc.te_user = d_eu.as<int32_t>(); Cc.te_movie = d_em.as<int32_t>(); Cc.te_rating = d_er.as<double>();
  Cc.N = (int)N; Cc.Ntest = (int)Ntest; Cc.w = d_w.as<double>(); Cc.U = d_U.as<double>();
  Cc.V = d_V.as<double>(); Cc.trainpred = d_trp.as<double>(); Cc.testpred = d_tep.as<double>();
  Cc.sse = d_sse.as<double>(); Cc.status = d_st.as<int32_t>();
  Cc.ymean = ytrainMean; Cc.ystd = ytrainStd;
  GPT_HIPCHK(d_ch.upload(&Cc, 1));
  // every output array starts at zero, and is zeroed again before the PosDefException error
  // (Julia throws: no outputs)
  auto zero_outputs = [&]() {
    if (w_store) std::memset(w_store, 0, 8 * rr * maxepoch);
    std::memset(U_store, 0, 8 * nU * maxepoch);
    std::memset(V_store, 0, 8 * nV * maxepoch);
    std::memset(testpred_store, 0, 8 * (size_t)Ntest * maxepoch);
    std::memset(trainRMSE, 0, 8 * (size_t)maxepoch);
    std::memset(testRMSE, 0, 8 * (size_t)maxepoch);
  };
  zero_outputs();
  // Kept sweeps are recorded on the device (w | U | V | test prediction | the two RMSEs per sweep,
  // up to ~1 GiB of sweeps at a time) and copied to the caller's arrays in chunks: no host
  // synchronisation inside a chunk (the round-4 loop copied and synchronised every sweep).
  const size_t kb = rr + nU + nV + (size_t)Ntest + 2;              // doubles per kept sweep
  const int64_t chunkE = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(maxepoch, 1),
                                                                 (int64_t)((1ull << 27) / kb)));
  GPT_HIPCHK(d_keep.alloc<double>(kb * chunkE));
  double* kw = d_keep.as<double>();
  double* kU = kw + rr * chunkE;
  double* kV = kU + nU * chunkE;
  double* ktp = kV + nV * chunkE;
  double* krm = ktp + (size_t)Ntest * chunkE;
  std::vector<double> rm(2 * (size_t)chunkE);
  int64_t flushed = 0;                              // kept sweeps already in the caller's arrays
  auto not_spd = [&]() -> int {
    zero_outputs();
    set_error("PosDefException: a Gibbs precision matrix is not positive definite");
    return GPT_ERR_NOT_SPD;
  };
  // The status word after every epoch's sweeps is copied into pinned memory behind them and read
  // one epoch later, so a failed Cholesky stops the sampler within two epochs without a full
  // synchronisation per epoch.
  struct StatusRing {
    int32_t* h = nullptr;
    hipEvent_t e[2] = {nullptr, nullptr};
    ~StatusRing() {
      for (auto x : e) if (x) (void)hipEventDestroy(x);
      if (h) (void)hipHostFree(h);
    }
  } sr;
  GPT_HIPCHK(hipHostMalloc((void**)&sr.h, 2 * sizeof(int32_t), hipHostMallocDefault));
  sr.h[0] = sr.h[1] = 0;
  for (auto& x : sr.e) GPT_HIPCHK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
  auto flush = [&](int64_t upto) -> int {
    GPT_HIPCHK(hipStreamSynchronize(nullptr));
    int32_t bad = 0;
    GPT_HIPCHK(d_st.download(&bad, 1));
    if (bad) return not_spd();
    const int64_t c = upto - flushed;
    if (c <= 0) return GPT_OK;
    if (w_store) GPT_HIPCHK(hipMemcpy(w_store + rr * flushed, kw, 8 * rr * c, hipMemcpyDeviceToHost));
    GPT_HIPCHK(hipMemcpy(U_store + nU * flushed, kU, 8 * nU * c, hipMemcpyDeviceToHost));
    GPT_HIPCHK(hipMemcpy(V_store + nV * flushed, kV, 8 * nV * c, hipMemcpyDeviceToHost));
    GPT_HIPCHK(hipMemcpy(testpred_store + (size_t)Ntest * flushed, ktp, 8 * (size_t)Ntest * c,
                         hipMemcpyDeviceToHost));
    GPT_HIPCHK(hipMemcpy(rm.data(), krm, 16 * c, hipMemcpyDeviceToHost));
    for (int64_t s2 = 0; s2 < c; ++s2) {
      trainRMSE[flushed + s2] = rm[2 * s2];
      testRMSE[flushed + s2] = rm[2 * s2 + 1];
    }
    flushed = upto;
    return GPT_OK;
  };
  const double su2 = sigma_u * sigma_u;
  int counter = 0;
  uint32_t sweep = 0;
  for (int64_t epoch = 1; epoch <= burnin + maxepoch; ++epoch) {
    for (int64_t g = 0; g < n_samples; ++g, ++sweep) {
      hipError_t e = launch_cfg_rows(0, (int)r, d_w.as<double>(), d_V.as<double>(), (int)n2,
                                     d_U.as<double>(), (int)n1, d_up.as<int32_t>(), d_ul.as<int32_t>(),
                                     d_tm.as<int32_t>(), d_tr.as<double>(), signal_var, su2, seed,
                                     sweep, kCfgU, d_st.as<int32_t>(), nullptr);
      if (e == hipSuccess)
        e = launch_cfg_rows(1, (int)r, d_w.as<double>(), d_U.as<double>(), (int)n1, d_V.as<double>(),
                            (int)n2, d_mp.as<int32_t>(), d_ml.as<int32_t>(), d_tu.as<int32_t>(),
                            d_tr.as<double>(), signal_var, su2, seed, sweep, kCfgV,
                            d_st.as<int32_t>(), nullptr);
      if (e == hipSuccess && !fixw)
        e = launch_cfg_wsystem((int)r, d_U.as<double>(), (int)n1, d_V.as<double>(), (int)n2,
                               d_up.as<int32_t>(), d_ul.as<int32_t>(), d_tm.as<int32_t>(),
                               d_tr.as<double>(), 1.0 / signal_var, 1.0 / (sigma_w * sigma_w),
                               1.0 / signal_var, d_ws.as<double>(), d_M.as<double>(),
                               d_x.as<double>(), nullptr);
      if (e == hipSuccess && !fixw)
        e = gaussian_draw_prec(d_M.as<double>(), p, d_x.as<double>(), seed, sweep, kCfgW, 0,
                               d_z.as<double>(), d_w.as<double>(), d_st.as<int32_t>(), nullptr);
      if (e != hipSuccess) return hip_fail(e, name);
    }
    if (epoch > burnin) {
      const int64_t s2 = epoch - burnin - 1, slot = (s2 - flushed);
      if (w_store) GPT_HIPCHK(hipMemcpyAsync(kw + rr * slot, d_w.p, 8 * rr, hipMemcpyDeviceToDevice, nullptr));
      GPT_HIPCHK(hipMemcpyAsync(kU + nU * slot, d_U.p, 8 * nU, hipMemcpyDeviceToDevice, nullptr));
      GPT_HIPCHK(hipMemcpyAsync(kV + nV * slot, d_V.p, 8 * nV, hipMemcpyDeviceToDevice, nullptr));
      if (!avg) counter = 0;
      hipError_t e = launch_cf_eval(P, d_ch.as<CfChain>(), 1, (int)std::max(N, Ntest), counter,
                                    nullptr);
      if (e == hipSuccess)
        e = launch_cfg_keep(d_ch.as<CfChain>(), (int)Ntest, neval, krm + 2 * slot,
                            ktp + (size_t)Ntest * slot, nullptr);
      if (e != hipSuccess) return hip_fail(e, "cf eval kernel");
      counter += 1;
      if (slot + 1 == chunkE) {
        const int rc = flush(s2 + 1);
        if (rc != GPT_OK) return rc;
      }
    }
    const int ring = (int)(epoch & 1);
    GPT_HIPCHK(hipMemcpyAsync(sr.h + ring, d_st.p, 4, hipMemcpyDeviceToHost, nullptr));
    GPT_HIPCHK(hipEventRecord(sr.e[ring], nullptr));
    if (epoch > 1) {                        // the previous epoch's status, one epoch behind
      GPT_HIPCHK(hipEventSynchronize(sr.e[ring ^ 1]));
      if (sr.h[ring ^ 1]) {
        GPT_HIPCHK(hipStreamSynchronize(nullptr));
        return not_spd();
      }
    }
  }
  return flush(maxepoch);
}

extern "C" int gpt_cf_fullw_gibbs(
    const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2, const double* Ratingtest,
    int64_t Ntest, int64_t ldt, double signal_var, double sigma_u, double sigma_w,
    const double* w_init, int64_t r, int64_t burnin, int64_t maxepoch, int64_t n_samples,
    uint64_t seed, double ytrainMean, double ytrainStd, int32_t avg, int32_t rotated_w,
    double* w_store, double* U_store, double* V_store, double* testpred_store, double* trainRMSE,
    double* testRMSE) {
  return cf_gibbs_run("GPT_fullw_gibbs", Rating, N, ldr, n1, n2, Ratingtest, Ntest, ldt,
                      signal_var, sigma_u, sigma_w, w_init, r, burnin, maxepoch, n_samples, seed,
                      ytrainMean, ytrainStd, avg, rotated_w, false, w_store, U_store, V_store,
                      testpred_store, trainRMSE, testRMSE);
}

extern "C" int gpt_cf_fixw_gibbs(
    const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2, const double* Ratingtest,
    int64_t Ntest, int64_t ldt, double signal_var, double sigma_u, const double* w, int64_t r,
    int64_t burnin, int64_t maxepoch, int64_t n_samples, uint64_t seed, double ytrainMean,
    double ytrainStd, int32_t avg, int32_t rotated_w, double* U_store, double* V_store,
    double* testpred_store, double* trainRMSE, double* testRMSE) {
  return cf_gibbs_run("GPT_fixw_gibbs", Rating, N, ldr, n1, n2, Ratingtest, Ntest, ldt,
                      signal_var, sigma_u, 1.0, w, r, burnin, maxepoch, n_samples, seed,
                      ytrainMean, ytrainStd, avg, rotated_w, true, nullptr, U_store, V_store,
                      testpred_store, trainRMSE, testRMSE);
}
