// MovieLens tensor CF from host arrays (100k_movielensExperiment.jl): the SGD / SGLD runs of the
// GPT_*w* variants over folds, and the Gibbs samplers.  Each C entry fills a CfModel, a CfSchedule
// and its folds by name and calls cf_sgd_run or cf_gibbs_run.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_util.h"

using namespace gpt;

// U, V initialisation of the SGD / SGLD CF samplers (the reference's variants differ):
//   kCfInitSide  GPT_fullw_sideinfo :424-428  stiefel ? polar(randn(r,rows)) : σ_u·randn(rows,r)
//   kCfInitSigma GPT_fixw / GPT_fixw_sideinfo :67 / :294  σ_u·randn(rows,r) (also when stiefel)
//   kCfInitUnit  GPT_fullw :175-180           stiefel ? polar(randn(r,rows)) : randn(rows,r)
enum CfInit { kCfInitSide = 0, kCfInitSigma = 1, kCfInitUnit = 2 };

// What the folds of a run share.  The defaults are the model without side information (D1 = D2 = 0
// with a = 1, b = c = 0) and the fixed-w variants' unused σ_w.
struct CfModel {
  const double* UserData = nullptr; int64_t n1 = 0, D1 = 0;
  const double* MovieData = nullptr; int64_t n2 = 0, D2 = 0;
  const double* w_init = nullptr; int64_t r = 0;
  double signal_var = 0.0, sigma_u = 0.0, sigma_w = 1.0, a = 1.0, b = 0.0, c = 0.0;
  uint64_t seed = 0;
  bool fixw = false;               // w stays at w_init (w_store may then be null)
  CfInit init = kCfInitSigma;
  int rowsU() const { return (int)(n1 + D1); }
  int rowsV() const { return (int)(n2 + D2); }
  bool masks() const { return D1 <= 64 && D2 <= 64; }
};
// How long and with which steps (m, eps*, langevin, stiefel: SGD's; n_samples, rotated_w: Gibbs's).
struct CfSchedule {
  int64_t m = 1, burnin = 0, maxepoch = 0, n_samples = 1;
  double epsw = 0.0, epsU = 0.0;
  int32_t langevin = 0, stiefel = 0, avg = 0, rotated_w = 0;
};
// One fold's ratings and outputs of a CF run (column-major, caller-owned).
struct CfFold {
  const double* Rating; int64_t N, ldr;
  const double* Ratingtest; int64_t Ntest, ldt;
  double ymean, ystd;
  double *w_store, *U_store, *V_store, *testpred_store, *trainRMSE, *testRMSE;
  int32_t status;                  // out: GPT_OK or GPT_ERR_NAN_GEODESIC
};
// Element counts of w, U and V, the kept epochs and the eval kernel's blocks per rating set.
struct CfSizes { size_t rr, nU, nV; int64_t maxepoch; int nmax, neval; };
static CfSizes cf_sizes(const CfModel& M, const CfSchedule& S, int64_t nmax) {
  return {(size_t)(M.r * M.r), (size_t)M.rowsU() * M.r, (size_t)M.rowsV() * M.r, S.maxepoch,
          (int)nmax, (int)((nmax + 255) / 256)};
}

// The parameter stores of a fold zeroed; with `curves` also its predictions and RMSE curves,
// testRMSE filled with `testRMSE_fill`.  An SGD run starts from 10.0 there (:441) and zeroes only
// the stores of a fold that bails out (:490-492); a Gibbs run starts from 0 and zeroes everything
// again before the PosDefException error (Julia throws: no outputs).
static void zero_outputs(const CfFold& f, const CfSizes& z, bool curves, double testRMSE_fill) {
  if (f.w_store) std::memset(f.w_store, 0, 8 * z.rr * z.maxepoch);
  std::memset(f.U_store, 0, 8 * z.nU * z.maxepoch);
  std::memset(f.V_store, 0, 8 * z.nV * z.maxepoch);
  if (!curves) return;
  std::memset(f.testpred_store, 0, 8 * (size_t)f.Ntest * z.maxepoch);
  std::memset(f.trainRMSE, 0, 8 * (size_t)z.maxepoch);
  std::fill(f.testRMSE, f.testRMSE + z.maxepoch, testRMSE_fill);
}

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

// 0-based user / movie ids and the ratings of a (count × 3, leading dimension ld) rating array, of
// a fold's training and test sets; the message when an id is outside the n1 users / n2 movies.
struct CfIds { std::vector<int32_t> user, movie; std::vector<double> rating; };
struct CfRatings { CfIds tr, te; };
static const char* cf_split_ratings(const double* R, int64_t count, int64_t ld, const CfModel& M,
                                    const char* what, CfIds& out) {
  out.user.resize(count); out.movie.resize(count); out.rating.resize(count);
  for (int64_t i = 0; i < count; ++i) {
    const int32_t u = out.user[i] = (int32_t)R[i] - 1, v = out.movie[i] = (int32_t)R[i + ld] - 1;
    out.rating[i] = R[i + 2 * ld];
    if (u < 0 || u >= M.n1 || v < 0 || v >= M.n2) return what;
  }
  return nullptr;
}
static const char* cf_split_fold(const CfFold& f, const CfModel& M, CfRatings& R) {
  const char* e = cf_split_ratings(f.Rating, f.N, f.ldr, M, "rating ids out of range", R.tr);
  return e ? e : cf_split_ratings(f.Ratingtest, f.Ntest, f.ldt, M, "test rating ids out of range", R.te);
}
// The bounds both samplers put on a fold and on the model.
static bool cf_fold_ok(const CfFold& f, bool fixw) {
  return f.Rating && f.Ratingtest && (fixw || f.w_store) && f.U_store && f.V_store &&
         f.testpred_store && f.trainRMSE && f.testRMSE && f.N >= 1 && f.Ntest >= 1 &&
         f.ldr >= f.N && f.ldt >= f.Ntest;
}
static bool cf_model_ok(const CfModel& M, const CfSchedule& S) {
  return M.w_init && M.n1 >= 1 && M.n2 >= 1 && S.burnin >= 0 && S.maxepoch >= 0 &&
         M.signal_var > 0 && M.sigma_u > 0 && M.sigma_w > 0;
}

// One fold's state on the device, of either sampler: ids, ratings, w, U, V, running predictions,
// SSE partials and status in one zeroed allocation, and the CfChain that points into it.  `sgd`
// adds the gradient rows GU / GV and the epoch-ordered copies of the training ratings.
struct CfFoldDev {
  DevMem blk;
  CfChain C{};
  void carve(Carve& k, const CfRatings& R, const CfSizes& z, bool sgd, const double* w0,
             const double* U0, const double* V0) {
    const size_t N = C.N, Nt = C.Ntest;
    C.tr_user = k.take(N, R.tr.user.data()); C.tr_movie = k.take(N, R.tr.movie.data());
    C.tr_rating = k.take(N, R.tr.rating.data());
    C.te_user = k.take(Nt, R.te.user.data()); C.te_movie = k.take(Nt, R.te.movie.data());
    C.te_rating = k.take(Nt, R.te.rating.data());
    C.w = k.take(z.rr, w0); C.U = k.take(z.nU, U0); C.V = k.take(z.nV, V0);
    C.trainpred = k.take<double>(N); C.testpred = k.take<double>(Nt);
    C.sse = k.take<double>(2 * (size_t)z.neval); C.status = k.take<int32_t>(1);
    if (!sgd) return;
    C.GU = k.take<double>(z.nU); C.GV = k.take<double>(z.nV);
    C.ep_user = k.take<int32_t>(N); C.ep_movie = k.take<int32_t>(N); C.ep_rating = k.take<double>(N);
  }
  int init(const CfFold& fd, const CfRatings& R, const CfSizes& z, bool sgd, const double* w0,
           const double* U0, const double* V0, const int32_t* perm) {
    C = CfChain{};
    C.N = (int)fd.N; C.Ntest = (int)fd.Ntest; C.ymean = fd.ymean; C.ystd = fd.ystd; C.perm = perm;
    Carve count, k;
    carve(count, R, z, sgd, w0, U0, V0);
    GPT_HIPCHK(blk.alloc<char>(count.off));
    GPT_HIPCHK(blk.zero());
    k.base = blk.as<char>();
    carve(k, R, z, sgd, w0, U0, V0);
    GPT_HIPCHK(k.err);
    return GPT_OK;
  }
};

// The side information on the device (each user's / movie's feature rows as CSR lists and, with
// `masks`, as one 64-bit mask) and the CfParams of a run of either sampler.
struct CfSideDev { DevMem up, uf, vp, vf, masks; };
static int fill_params(const CfModel& M, const CfSchedule& S, bool masks, CfSideDev& d, CfParams& P) {
  const int64_t n1 = M.n1, n2 = M.n2;
  std::vector<int32_t> uptr, ufe, vptr, vfe;
  cf_features(M.UserData, (int)n1, (int)M.D1, (int)n1, uptr, ufe);
  cf_features(M.MovieData, (int)n2, (int)M.D2, (int)n2, vptr, vfe);
  GPT_HIPCHK(d.up.upload(uptr.data(), uptr.size()));
  GPT_HIPCHK(d.uf.upload(ufe.data(), ufe.size()));
  GPT_HIPCHK(d.vp.upload(vptr.data(), vptr.size()));
  GPT_HIPCHK(d.vf.upload(vfe.data(), vfe.size()));
  P = CfParams{};
  P.n1 = (int)n1; P.D1 = (int)M.D1; P.n2 = (int)n2; P.D2 = (int)M.D2; P.r = (int)M.r; P.m = (int)S.m;
  P.rowsU = M.rowsU(); P.rowsV = M.rowsV();
  P.a = M.a; P.b = M.b; P.c = M.c;
  P.signal_var = M.signal_var; P.sigma_u = M.sigma_u; P.sigma_w = M.sigma_w;
  P.epsw = S.epsw; P.epsU = S.epsU; P.langevin = S.langevin; P.stiefel = S.stiefel;
  P.seed = M.seed; P.fixw = M.fixw ? 1 : 0;
  P.uptr = d.up.as<int32_t>(); P.ufe = d.uf.as<int32_t>();
  P.vptr = d.vp.as<int32_t>(); P.vfe = d.vf.as<int32_t>();
  if (!masks) return GPT_OK;
  std::vector<uint64_t> mk((size_t)(n1 + n2), 0);
  for (int64_t i = 0; i < n1; ++i)
    for (int z = uptr[i]; z < uptr[i + 1]; ++z) mk[i] |= 1ull << (ufe[z] - n1);
  for (int64_t i = 0; i < n2; ++i)
    for (int z = vptr[i]; z < vptr[i + 1]; ++z) mk[n1 + i] |= 1ull << (vfe[z] - n2);
  GPT_HIPCHK(d.masks.upload(mk.data(), mk.size()));
  P.umask = d.masks.as<uint64_t>();
  P.vmask = P.umask + n1;
  return GPT_OK;
}

// ---- SGD / SGLD -------------------------------------------------------------------------------
// Device time of the last CF SGD run on this thread (gpt_cf_last_timing): hipEvents around each
// epoch / eval launch, read after the per-epoch status copy that synchronises anyway.
struct CfTiming { double epoch_ms, eval_ms; int64_t epochs, evals, fold_steps; };
static thread_local CfTiming g_cf_timing{};
static thread_local CfMode g_cf_mode = kCfStepPairs;      // gpt_cf_last_mode
// GPTSGLD_CF_STAMPS=1: per-phase s_memtime of fold 0's first epoch (gpt_cf_last_stamps)
static thread_local std::vector<long long> g_cf_stamps;
// gpt_debug_cf_init's one-shot initial state of the next CF SGD run on this thread
struct CfInject { bool armed = false; int64_t rowsU = 0, rowsV = 0, r = 0; std::vector<double> U, V; };
static thread_local CfInject g_cf_inject;

// The message of the first bad argument of an SGD run, or none.
static std::string cf_sgd_check(const char* name, const CfModel& M, const CfSchedule& S,
                                const std::vector<CfFold>& folds, const CfInject& inj) {
  bool ok = !folds.empty() && (M.D1 == 0 || M.UserData) && (M.D2 == 0 || M.MovieData) &&
            M.D1 >= 0 && M.D2 >= 0 && S.m >= 1 && cf_model_ok(M, S);
  for (const CfFold& f : folds) ok = ok && cf_fold_ok(f, M.fixw) && f.N == folds[0].N;
  if (!ok) return std::string("bad ") + name + " arguments";
  if (!rank_supported((int)M.r) ||
      cf_lds_bytes((int)M.r, (int)S.m, (int)(M.D1 + M.D2), M.masks()) > kMaxLds)
    return std::string(name) + ": rank not instantiated (" + ranks_text() + ") or minibatch too large";
  if (inj.armed && (inj.rowsU != M.rowsU() || inj.rowsV != M.rowsV() || inj.r != M.r))
    return std::string(name) + ": the injected U0 / V0 (gpt_debug_cf_init) are " +
           std::to_string(inj.rowsU) + " and " + std::to_string(inj.rowsV) + " rows of rank " +
           std::to_string(inj.r) + ", the run has " + std::to_string(M.rowsU()) + " and " +
           std::to_string(M.rowsV()) + " of rank " + std::to_string(M.r);
  return "";
}
// The initial U (which = 0) or V (1) of an SGD run: see CfInit.
static std::vector<double> cf_init_uv(const CfModel& M, bool stiefel, int which) {
  const int rows = which ? M.rowsV() : M.rowsU();
  std::vector<double> Z((size_t)rows * M.r), out(Z.size());
  for (size_t e = 0; e < Z.size(); ++e) Z[e] = host_normal(M.seed, (uint32_t)e, 0, kCfUVInit, (uint32_t)which);
  if (stiefel && M.init != kCfInitSigma) host_stiefel_polar(Z.data(), (int)M.r, rows, out.data());
  else if (M.init == kCfInitUnit) out = Z;
  else for (size_t e = 0; e < Z.size(); ++e) out[e] = M.sigma_u * Z[e];
  return out;
}
// How an epoch goes to the device.  The Stiefel move needs Grams over every row and the lazy move
// of SGD (no Langevin noise, no Stiefel geometry) on the feature-mask path none of the rows outside
// the batch: the whole epoch in one workgroup per fold, one launch.  GPTSGLD_CF_LAZY=0 keeps the
// batch-phase / move launch pairs.
// (the decay factor c = 1 − εU/(2σ_u²) of a skipped row must lie in (0, 1): the kernel reads a row
// Δ steps behind as m·c^Δ; outside that range the eager move keeps the reference's numbers)
static CfMode cf_pick_mode(const CfSchedule& S, const CfParams& P, int nbatch) {
  if (S.stiefel) return kCfStiefelEpoch;
  const double cdecay = 1.0 - P.epsU / (2.0 * P.sigma_u * P.sigma_u);
  const char* env = std::getenv("GPTSGLD_CF_LAZY");
  const bool lazy = !S.langevin && P.umask != nullptr && cdecay > 0.0 && cdecay < 1.0 &&
                    cf_lazy_lds_bytes(P.r, P.m, P.D1 + P.D2, P.rowsU + P.rowsV, nbatch) <= kMaxLds &&
                    !(env && std::strcmp(env, "0") == 0);
  return lazy ? kCfLazyEpoch : kCfStepPairs;
}

// The run's own stream and what it launches per epoch: the gather, then the epoch launch
// (kCfStiefelEpoch, kCfLazyEpoch) or, in kCfStepPairs, per minibatch the batch phase (one workgroup
// per fold) and the row-parallel move of U and V over the whole GPU (cf_move_kernel) — an epoch of
// them as one captured graph, its steps counted from a device-side epoch base.
struct CfEpochLauncher {
  CfMode mode;
  const CfParams& P;               // the run's: its stamp buffer goes after the first epoch
  const CfChain* chains;
  int F, N, nbatch;
  hipStream_t s = nullptr;
  hipGraph_t g = nullptr; hipGraphExec_t x = nullptr;
  DevMem step;                     // the graph replays' epoch base
  long long step_base_host = 0;    // read by the copy to `step`, alive until the epoch's event sync
  ~CfEpochLauncher() {
    if (s) (void)hipStreamSynchronize(s);
    if (x) (void)hipGraphExecDestroy(x);
    if (g) (void)hipGraphDestroy(g);
    if (s) (void)hipStreamDestroy(s);
  }
  int init() {
    GPT_HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    GPT_HIPCHK(hipStreamSynchronize(nullptr));         // the set-up copies / memsets are done
    GPT_HIPCHK(step.alloc<long long>(1));
    return GPT_OK;
  }
  // the epoch's launches, its steps counted from step0 (plus *base on the device)
  hipError_t enqueue(long long step0, const long long* base) {
    hipError_t e = launch_cf_gather(chains, F, N, s);
    if (mode != kCfStepPairs)
      return e != hipSuccess ? e : launch_cf_epoch(P, chains, F, step0, 0, nbatch, mode, s);
    for (int b = 0; b < nbatch && e == hipSuccess; ++b) {
      e = launch_cf_epoch(P, chains, F, step0 + b, b, 1, kCfStepPairs, s, base);
      if (e == hipSuccess) e = launch_cf_move(P, chains, F, step0 + b, s, base);
    }
    return e;
  }
  // One epoch on the stream behind `begin`: direct launches, but a replay of the step pairs' graph
  // (their stamped first epoch goes directly: the stamp buffer is dropped after it).
  int launch(int64_t epoch, hipEvent_t begin) {
    const long long step0 = (epoch - 1) * nbatch;
    hipError_t e;
    if (mode != kCfStepPairs || P.stamps) {
      GPT_HIPCHK(hipEventRecord(begin, s));
      e = enqueue(step0, nullptr);
    } else {
      if (!x) {
        GPT_HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        e = enqueue(0, step.as<long long>());
        const hipError_t ec = hipStreamEndCapture(s, &g);
        if (e != hipSuccess) return hip_fail(e, "cf epoch capture");
        if (ec != hipSuccess) return hip_fail(ec, "hipStreamEndCapture");
        GPT_HIPCHK(hipGraphInstantiate(&x, g, nullptr, nullptr, 0));
      }
      step_base_host = step0;
      GPT_HIPCHK(hipMemcpyAsync(step.p, &step_base_host, sizeof(long long), hipMemcpyHostToDevice, s));
      GPT_HIPCHK(hipEventRecord(begin, s));
      e = hipGraphLaunch(x, s);
    }
    return e != hipSuccess ? hip_fail(e, "cf epoch kernel") : GPT_OK;
  }
};
// `end` recorded on st and waited for; the device time since `begin` added to *ms.
static int cf_stop_timer(hipEvent_t begin, hipEvent_t end, hipStream_t st, double* ms) {
  GPT_HIPCHK(hipEventRecord(end, st));
  GPT_HIPCHK(hipEventSynchronize(end));
  float t = 0.f;
  GPT_HIPCHK(hipEventElapsedTime(&t, begin, end));
  *ms += t;
  return GPT_OK;
}

// The folds of an SGD run: the caller's outputs, the device state and who is still running.
struct CfSgdFolds {
  std::vector<CfFold>& folds;
  CfSizes z;
  std::vector<CfFoldDev> dev;
  std::vector<char> live;
  std::vector<int> rises;          // test RMSE rises in a row (testcounter of :541-547)
  int nlive;
  std::vector<double> sse, tp;     // an epoch's SSE partials and test predictions of one fold
  CfSgdFolds(std::vector<CfFold>& folds_, const CfSizes& z_, int64_t ntmax)
      : folds(folds_), z(z_), dev(folds_.size()), live(folds_.size(), 1), rises(folds_.size(), 0),
        nlive((int)folds_.size()), sse(2 * (size_t)z_.neval), tp(ntmax) {}
  void retire(int f) { live[f] = 0; --nlive; }
  // A fold whose geodesic gave NaN in this epoch (:490-492): zero parameter stores, curves kept.
  int poll_bails() {
    for (size_t f = 0; f < folds.size(); ++f) {
      if (!live[f]) continue;
      int32_t bad = 0;
      GPT_HIPCHK(hipMemcpy(&bad, dev[f].C.status, 4, hipMemcpyDeviceToHost));
      if (!bad) continue;
      zero_outputs(folds[f], z, false, 0.0);
      folds[f].status = GPT_ERR_NAN_GEODESIC;
      retire((int)f);
    }
    return GPT_OK;
  }
  // Kept epoch s2 of every live fold: the sample, the RMSEs from the eval kernel's partial sums
  // (added in order), the clipped test predictions, and the early stop — a status of 2 skips the
  // fold in later launches.
  int keep(int64_t epoch, int64_t s2) {
    const int32_t stopped = 2;
    for (size_t f = 0; f < folds.size(); ++f) {
      if (!live[f]) continue;
      CfFold& fd = folds[f];
      const CfChain& C = dev[f].C;
      if (fd.w_store) GPT_HIPCHK(hipMemcpy(fd.w_store + z.rr * s2, C.w, 8 * z.rr, hipMemcpyDeviceToHost));
      GPT_HIPCHK(hipMemcpy(fd.U_store + z.nU * s2, C.U, 8 * z.nU, hipMemcpyDeviceToHost));
      GPT_HIPCHK(hipMemcpy(fd.V_store + z.nV * s2, C.V, 8 * z.nV, hipMemcpyDeviceToHost));
      GPT_HIPCHK(hipMemcpy(sse.data(), C.sse, 16 * (size_t)z.neval, hipMemcpyDeviceToHost));
      GPT_HIPCHK(hipMemcpy(tp.data(), C.testpred, 8 * fd.Ntest, hipMemcpyDeviceToHost));
      double st0 = 0.0, st1 = 0.0;
      for (int e = 0; e < z.neval; ++e) { st0 += sse[2 * e]; st1 += sse[2 * e + 1]; }
      fd.trainRMSE[s2] = std::sqrt(st0 / (double)fd.N);
      fd.testRMSE[s2] = std::sqrt(st1 / (double)fd.Ntest);
      for (int64_t i = 0; i < fd.Ntest; ++i)
        fd.testpred_store[(size_t)fd.Ntest * s2 + i] =
            std::min(std::max(tp[i] * fd.ystd + fd.ymean, 1.0), 5.0);
      // :541-547 (the reference compares with the previous epoch's entry; none at s2 = 0)
      if (epoch > 1 && s2 > 0 && fd.testRMSE[s2] > fd.testRMSE[s2 - 1]) rises[f] += 1;
      else rises[f] = 0;
      if (rises[f] >= 5) {
        GPT_HIPCHK(hipMemcpy(C.status, &stopped, 4, hipMemcpyHostToDevice));
        retire((int)f);
      }
    }
    return GPT_OK;
  }
};

// SGD / SGLD runs of the tensor CF model (the body of every GPT_*w* SGD variant) for F folds at
// once: sibling chains of one launch per epoch (the reference's `@parallel for i=1:5`, :733-736),
// each with its own ratings, state, evaluation and early stop; a fold that stops or bails out is
// skipped by later launches.  The folds share the model, hence the initial U, V (as separate calls
// with one param_seed do), the per-epoch permutation and the number of training ratings.  Every
// argument and every rating id is checked before the first device call.
static int cf_sgd_run(const char* name, const CfModel& M, const CfSchedule& S, std::vector<CfFold>& folds) {
  CfInject inj;                                      // taken here: cleared however the run ends
  std::swap(inj, g_cf_inject);
  std::string err = cf_sgd_check(name, M, S, folds, inj);
  std::vector<CfRatings> split(folds.size());
  for (size_t f = 0; f < folds.size() && err.empty(); ++f)
    if (const char* e = cf_split_fold(folds[f], M, split[f])) err = e;
  if (!err.empty()) { set_error(err); return GPT_ERR_BAD_DIMS; }
  const int F = (int)folds.size(), N = (int)folds[0].N, nbatch = (int)((N + S.m - 1) / S.m);
  int64_t ntmax = 0;
  for (const CfFold& f : folds) ntmax = std::max(ntmax, f.Ntest);
  CfSgdFolds R(folds, cf_sizes(M, S, std::max<int64_t>(N, ntmax)), ntmax);
  const std::vector<double> U0 = inj.armed ? inj.U : cf_init_uv(M, S.stiefel, 0);
  const std::vector<double> V0 = inj.armed ? inj.V : cf_init_uv(M, S.stiefel, 1);
  DevMem d_perm, d_ch, d_stamps;
  GPT_HIPCHK(d_perm.alloc<int32_t>(N));
  std::vector<CfChain> ch(F);
  for (int f = 0; f < F; ++f) {
    GPT_TRY(R.dev[f].init(folds[f], split[f], R.z, true, M.w_init, U0.data(), V0.data(), d_perm.as<int32_t>()));
    ch[f] = R.dev[f].C;
    zero_outputs(folds[f], R.z, true, 10.0);
    folds[f].status = GPT_OK;
  }
  GPT_HIPCHK(d_ch.upload(ch.data(), ch.size()));
  CfSideDev side; CfParams P;
  GPT_TRY(fill_params(M, S, M.masks(), side, P));
  g_cf_stamps.clear();
  if (std::getenv("GPTSGLD_CF_STAMPS")) {
    GPT_HIPCHK(d_stamps.alloc<long long>((size_t)kCfStampSteps * kCfStampSlots));
    GPT_HIPCHK(d_stamps.zero());
    P.stamps = d_stamps.as<long long>();
  }
#if CF_WSTAMPS
  if (std::getenv("GPTSGLD_CF_EXP")) P.exp = std::atoi(std::getenv("GPTSGLD_CF_EXP"));
#endif
  std::vector<int32_t> perm(N);
  int counter = 0;                 // evaluations in the running average
  ScopedEvents evs;
  GPT_HIPCHK(evs.create(4));
  CfEpochLauncher L{cf_pick_mode(S, P, nbatch), P, d_ch.as<CfChain>(), F, N, nbatch};
  GPT_TRY(L.init());
  g_cf_timing = CfTiming{};
  g_cf_mode = L.mode;
  for (int64_t epoch = 1; epoch <= S.burnin + S.maxepoch && R.nlive > 0; ++epoch) {
    host_randperm(N, M.seed, (int)(epoch - 1), perm.data());
    GPT_HIPCHK(hipMemcpy(d_perm.p, perm.data(), d_perm.bytes, hipMemcpyHostToDevice));
    GPT_TRY(L.launch(epoch, evs.e[0]));
    GPT_TRY(cf_stop_timer(evs.e[0], evs.e[1], L.s, &g_cf_timing.epoch_ms));
    if (P.stamps) {                // the first epoch only
      g_cf_stamps.resize((size_t)kCfStampSteps * kCfStampSlots);
      GPT_HIPCHK(d_stamps.download(g_cf_stamps.data(), g_cf_stamps.size()));
      P.stamps = nullptr;
    }
    g_cf_timing.epochs += 1;
    g_cf_timing.fold_steps += (int64_t)R.nlive * nbatch;
    GPT_TRY(R.poll_bails());
    if (epoch <= S.burnin || R.nlive == 0) continue;
    if (!S.avg) counter = 0;
    GPT_HIPCHK(hipEventRecord(evs.e[2], L.s));
    const hipError_t e = launch_cf_eval(P, d_ch.as<CfChain>(), F, R.z.nmax, counter, L.s);
    if (e != hipSuccess) return hip_fail(e, "cf eval kernel");
    GPT_TRY(cf_stop_timer(evs.e[2], evs.e[3], L.s, &g_cf_timing.eval_ms));
    g_cf_timing.evals += 1;
    GPT_TRY(R.keep(epoch, epoch - S.burnin - 1));
    counter += 1;
  }
  for (const CfFold& fd : folds)
    if (fd.status != GPT_OK) {
      set_error("Get NaN when moving along Geodesic. Try smaller epsU");
      return GPT_ERR_NAN_GEODESIC;
    }
  return GPT_OK;
}

extern "C" int gpt_cf_fullw_sideinfo(
    const double* Rating, int64_t N, int64_t ldr, const double* UserData, int64_t n1, int64_t D1,
    const double* MovieData, int64_t n2, int64_t D2, const double* Ratingtest, int64_t Ntest,
    int64_t ldt, double signal_var, double sigma_u, double sigma_w, const double* w_init, int64_t r,
    int64_t m, double epsw, double epsU, double a, double b, double c, int64_t burnin,
    int64_t maxepoch, uint64_t seed, double ytrainMean, double ytrainStd, int32_t langevin,
    int32_t stiefel, int32_t avg, double* w_store, double* U_store, double* V_store,
    double* testpred_store, double* trainRMSE, double* testRMSE) {
  CfModel M;
  M.UserData = UserData; M.n1 = n1; M.D1 = D1; M.MovieData = MovieData; M.n2 = n2; M.D2 = D2;
  M.r = r; M.signal_var = signal_var; M.sigma_u = sigma_u; M.sigma_w = sigma_w; M.w_init = w_init;
  M.a = a; M.b = b; M.c = c; M.seed = seed; M.init = kCfInitSide;
  CfSchedule S;
  S.m = m; S.epsw = epsw; S.epsU = epsU; S.burnin = burnin; S.maxepoch = maxepoch;
  S.langevin = langevin; S.stiefel = stiefel; S.avg = avg;
  std::vector<CfFold> folds{{Rating, N, ldr, Ratingtest, Ntest, ldt, ytrainMean, ytrainStd, w_store,
                             U_store, V_store, testpred_store, trainRMSE, testRMSE, GPT_OK}};
  return cf_sgd_run("GPT_fullw_sideinfo", M, S, folds);
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
  CfModel M;
  M.UserData = UserData; M.n1 = n1; M.D1 = D1; M.MovieData = MovieData; M.n2 = n2; M.D2 = D2;
  M.r = r; M.signal_var = signal_var; M.sigma_u = sigma_u; M.sigma_w = sigma_w; M.w_init = w_init;
  M.a = a; M.b = b; M.c = c; M.seed = seed; M.init = kCfInitSide;
  CfSchedule S;
  S.m = m; S.epsw = epsw; S.epsU = epsU; S.burnin = burnin; S.maxepoch = maxepoch;
  S.langevin = langevin; S.stiefel = stiefel; S.avg = avg;
  std::vector<CfFold> folds(F);
  for (int64_t f = 0; f < F; ++f)
    folds[f] = CfFold{Rating[f], N[f], N[f], Ratingtest[f], Ntest[f], Ntest[f], ytrainMean[f],
                      ytrainStd[f], w_store[f], U_store[f], V_store[f], testpred_store[f],
                      trainRMSE[f], testRMSE[f], GPT_OK};
  const int rc = cf_sgd_run("GPT_fullw_sideinfo_folds", M, S, folds);
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
  *epoch_ms = g_cf_timing.epoch_ms; *eval_ms = g_cf_timing.eval_ms;
  *epochs = g_cf_timing.epochs; *fold_steps = g_cf_timing.fold_steps;
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
  CfModel M;
  M.UserData = UserData; M.n1 = n1; M.D1 = D1; M.MovieData = MovieData; M.n2 = n2; M.D2 = D2;
  M.r = r; M.signal_var = signal_var; M.sigma_u = sigma_u; M.w_init = w;
  M.a = a; M.b = b; M.c = c; M.seed = seed; M.fixw = true; M.init = kCfInitSigma;
  CfSchedule S;
  S.m = m; S.epsU = epsU; S.burnin = burnin; S.maxepoch = maxepoch;
  S.langevin = langevin; S.stiefel = stiefel; S.avg = avg;
  std::vector<CfFold> folds{{Rating, N, ldr, Ratingtest, Ntest, ldt, ytrainMean, ytrainStd, nullptr,
                             U_store, V_store, testpred_store, trainRMSE, testRMSE, GPT_OK}};
  return cf_sgd_run("GPT_fixw_sideinfo", M, S, folds);
}

extern "C" int gpt_cf_fullw(const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
                            const double* Ratingtest, int64_t Ntest, int64_t ldt,
                            double signal_var, double sigma_u, double sigma_w,
                            const double* w_init, int64_t r, int64_t m, double epsw, double epsU,
                            int64_t burnin, int64_t maxepoch, uint64_t seed, double ytrainMean,
                            double ytrainStd, int32_t langevin, int32_t stiefel, int32_t avg,
                            double* w_store, double* U_store, double* V_store,
                            double* testpred_store, double* trainRMSE, double* testRMSE) {
  CfModel M;
  M.n1 = n1; M.n2 = n2; M.r = r; M.signal_var = signal_var; M.sigma_u = sigma_u;
  M.sigma_w = sigma_w; M.w_init = w_init; M.seed = seed; M.init = kCfInitUnit;
  CfSchedule S;
  S.m = m; S.epsw = epsw; S.epsU = epsU; S.burnin = burnin; S.maxepoch = maxepoch;
  S.langevin = langevin; S.stiefel = stiefel; S.avg = avg;
  std::vector<CfFold> folds{{Rating, N, ldr, Ratingtest, Ntest, ldt, ytrainMean, ytrainStd, w_store,
                             U_store, V_store, testpred_store, trainRMSE, testRMSE, GPT_OK}};
  return cf_sgd_run("GPT_fullw", M, S, folds);
}

extern "C" int gpt_cf_fixw(const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
                           const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var,
                           double sigma_u, const double* w, int64_t r, int64_t m, double epsU,
                           int64_t burnin, int64_t maxepoch, uint64_t seed, double ytrainMean,
                           double ytrainStd, int32_t langevin, int32_t stiefel, int32_t avg,
                           double* U_store, double* V_store, double* testpred_store,
                           double* trainRMSE, double* testRMSE) {
  CfModel M;
  M.n1 = n1; M.n2 = n2; M.r = r; M.signal_var = signal_var; M.sigma_u = sigma_u; M.w_init = w;
  M.seed = seed; M.fixw = true; M.init = kCfInitSigma;
  CfSchedule S;
  S.m = m; S.epsU = epsU; S.burnin = burnin; S.maxepoch = maxepoch;
  S.langevin = langevin; S.stiefel = stiefel; S.avg = avg;
  std::vector<CfFold> folds{{Rating, N, ldr, Ratingtest, Ntest, ldt, ytrainMean, ytrainStd, nullptr,
                             U_store, V_store, testpred_store, trainRMSE, testRMSE, GPT_OK}};
  return cf_sgd_run("GPT_fixw", M, S, folds);
}

// ---- Gibbs -------------------------------------------------------------------------------------
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

// The initial state of a Gibbs run (:1047-1053): Q = qr(randn(r,r)), U = σ_u·randn(n1,r),
// V = σ_u·randn(n2,r), w = w_init; rotated: w = Q·w_init, U = U·Q'.
static void cfg_init(const CfModel& M, bool rotated_w, std::vector<double>& w0,
                     std::vector<double>& U0, std::vector<double>& V0) {
  const int64_t r = M.r, n1 = M.n1;
  const size_t rr = (size_t)r * r;
  std::vector<double> Qm(rr);
  w0.assign(M.w_init, M.w_init + rr); U0.resize((size_t)n1 * r); V0.resize((size_t)M.n2 * r);
  for (size_t e = 0; e < rr; ++e) Qm[e] = host_normal(M.seed, (uint32_t)e, 0, kCfgInit, 0);
  for (size_t e = 0; e < U0.size(); ++e) U0[e] = M.sigma_u * host_normal(M.seed, (uint32_t)e, 0, kCfgInit, 1);
  for (size_t e = 0; e < V0.size(); ++e) V0[e] = M.sigma_u * host_normal(M.seed, (uint32_t)e, 0, kCfgInit, 2);
  if (!rotated_w) return;
  host_qr_q((int)r, Qm);
  for (int64_t i = 0; i < r; ++i)
    for (int64_t j = 0; j < r; ++j) {
      double s = 0.0;
      for (int64_t k = 0; k < r; ++k) s += Qm[i + r * k] * M.w_init[k + r * j];
      w0[i + r * j] = s;
    }
  std::vector<double> U1(U0.size());
  for (int64_t i = 0; i < n1; ++i)
    for (int64_t j = 0; j < r; ++j) {
      double s = 0.0;
      for (int64_t k = 0; k < r; ++k) s += U0[i + n1 * k] * Qm[j + r * k];
      U1[i + n1 * j] = s;
    }
  U0.swap(U1);
}

// What a Gibbs run keeps on the device beside its fold: the ratings of each user / movie as CSR
// lists in Rating order (idx = (Rating[:,1].==i), :1061), the w system M / x / z and its scratch.
struct CfGibbsDev {
  DevMem up, mp, ul, ml, M, x, z, ws;
  int init(const CfModel& Md, const CfRatings& R) {
    const std::vector<int32_t>&tu = R.tr.user, &tm = R.tr.movie;
    const int64_t N = (int64_t)tu.size(), n1 = Md.n1, n2 = Md.n2;
    std::vector<int32_t> uptr(n1 + 1, 0), mptr(n2 + 1, 0), ulst(N), mlst(N);
    for (int64_t i = 0; i < N; ++i) { uptr[tu[i] + 1]++; mptr[tm[i] + 1]++; }
    for (int64_t i = 0; i < n1; ++i) uptr[i + 1] += uptr[i];
    for (int64_t i = 0; i < n2; ++i) mptr[i + 1] += mptr[i];
    std::vector<int32_t> cu(uptr.begin(), uptr.end() - 1), cm(mptr.begin(), mptr.end() - 1);
    for (int64_t i = 0; i < N; ++i) { ulst[cu[tu[i]]++] = (int32_t)i; mlst[cm[tm[i]]++] = (int32_t)i; }
    const size_t rr = (size_t)(Md.r * Md.r);
    GPT_HIPCHK(up.upload(uptr.data(), uptr.size()));
    GPT_HIPCHK(mp.upload(mptr.data(), mptr.size()));
    GPT_HIPCHK(ul.upload(ulst.data(), ulst.size()));
    GPT_HIPCHK(ml.upload(mlst.data(), mlst.size()));
    GPT_HIPCHK(M.alloc<double>(rr * rr));
    GPT_HIPCHK(x.alloc<double>(rr));
    GPT_HIPCHK(z.alloc<double>(rr));
    GPT_HIPCHK(ws.alloc<double>(cfg_wsystem_scratch_dbl((int)Md.r, (int)n1)));
    return GPT_OK;
  }
};

// One sweep: the user rows, the movie rows and, unless w is fixed, w | U, V.
static hipError_t cfg_sweep(const CfModel& M, const CfChain& C, const CfGibbsDev& G, uint32_t sweep) {
  const int r = (int)M.r, n1 = (int)M.n1, n2 = (int)M.n2;
  const double su2 = M.sigma_u * M.sigma_u;
  hipError_t e = launch_cfg_rows(0, r, C.w, C.V, n2, C.U, n1, G.up.as<int32_t>(), G.ul.as<int32_t>(),
                                 C.tr_movie, C.tr_rating, M.signal_var, su2, M.seed, sweep, kCfgU,
                                 C.status, nullptr);
  if (e == hipSuccess)
    e = launch_cfg_rows(1, r, C.w, C.U, n1, C.V, n2, G.mp.as<int32_t>(), G.ml.as<int32_t>(),
                        C.tr_user, C.tr_rating, M.signal_var, su2, M.seed, sweep, kCfgV, C.status,
                        nullptr);
  if (e == hipSuccess && !M.fixw)
    e = launch_cfg_wsystem(r, C.U, n1, C.V, n2, G.up.as<int32_t>(), G.ul.as<int32_t>(), C.tr_movie,
                           C.tr_rating, 1.0 / M.signal_var, 1.0 / (M.sigma_w * M.sigma_w),
                           1.0 / M.signal_var, G.ws.as<double>(), G.M.as<double>(),
                           G.x.as<double>(), nullptr);
  if (e == hipSuccess && !M.fixw)
    e = gaussian_draw_prec(G.M.as<double>(), r * r, G.x.as<double>(), M.seed, sweep, kCfgW, 0,
                           G.z.as<double>(), C.w, C.status, nullptr);
  return e;
}
static int cfg_not_spd(const CfFold& fd, const CfSizes& z) {
  zero_outputs(fd, z, true, 0.0);
  set_error("PosDefException: a Gibbs precision matrix is not positive definite");
  return GPT_ERR_NOT_SPD;
}
// Kept sweeps are recorded on the device (w | U | V | test prediction | the two RMSEs per sweep,
// up to ~1 GiB of sweeps at a time) and copied to the caller's arrays in chunks: no host
// synchronisation inside a chunk.
struct CfKeep {
  DevMem buf;
  double *w, *U, *V, *tp, *rm;
  int64_t chunkE, flushed = 0;     // sweeps per chunk; kept sweeps already in the caller's arrays
  std::vector<double> rmh;
  int init(const CfSizes& z, int64_t Ntest) {
    const size_t kb = z.rr + z.nU + z.nV + (size_t)Ntest + 2;              // doubles per kept sweep
    chunkE = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(z.maxepoch, 1),
                                                     (int64_t)((1ull << 27) / kb)));
    GPT_HIPCHK(buf.alloc<double>(kb * chunkE));
    w = buf.as<double>(); U = w + z.rr * chunkE; V = U + z.nU * chunkE;
    tp = V + z.nV * chunkE; rm = tp + (size_t)Ntest * chunkE;
    rmh.resize(2 * (size_t)chunkE);
    return GPT_OK;
  }
  // the kept sweeps flushed .. upto - 1 into the caller's arrays, after the run's status
  int flush(const CfFold& fd, const CfSizes& z, const int32_t* status, int64_t upto) {
    GPT_HIPCHK(hipStreamSynchronize(nullptr));
    int32_t bad = 0;
    GPT_HIPCHK(hipMemcpy(&bad, status, 4, hipMemcpyDeviceToHost));
    if (bad) return cfg_not_spd(fd, z);
    const int64_t c = upto - flushed;
    if (c <= 0) return GPT_OK;
    if (fd.w_store) GPT_HIPCHK(hipMemcpy(fd.w_store + z.rr * flushed, w, 8 * z.rr * c, hipMemcpyDeviceToHost));
    GPT_HIPCHK(hipMemcpy(fd.U_store + z.nU * flushed, U, 8 * z.nU * c, hipMemcpyDeviceToHost));
    GPT_HIPCHK(hipMemcpy(fd.V_store + z.nV * flushed, V, 8 * z.nV * c, hipMemcpyDeviceToHost));
    GPT_HIPCHK(hipMemcpy(fd.testpred_store + fd.Ntest * flushed, tp, 8 * fd.Ntest * c, hipMemcpyDeviceToHost));
    GPT_HIPCHK(hipMemcpy(rmh.data(), rm, 16 * c, hipMemcpyDeviceToHost));
    for (int64_t s2 = 0; s2 < c; ++s2) {
      fd.trainRMSE[flushed + s2] = rmh[2 * s2];
      fd.testRMSE[flushed + s2] = rmh[2 * s2 + 1];
    }
    flushed = upto;
    return GPT_OK;
  }
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
  int init() {
    GPT_HIPCHK(hipHostMalloc((void**)&h, 2 * sizeof(int32_t), hipHostMallocDefault));
    h[0] = h[1] = 0;
    for (auto& x : e) GPT_HIPCHK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
    return GPT_OK;
  }
};
static std::string cf_gibbs_check(const char* name, const CfModel& M, const CfSchedule& S, const CfFold& fd) {
  if (!cf_fold_ok(fd, M.fixw) || !cf_model_ok(M, S) || S.n_samples < 1)
    return std::string("bad ") + name + " arguments";
  if (!rank_supported((int)M.r) || M.r * M.r > 1024)
    return std::string(name) + ": rank not instantiated (" + ranks_text() + ")";
  return "";
}

// Gibbs sweeps of the CF model without side information (GPT_fullw_gibbs; fixw: GPT_fixw_gibbs,
// :945-1028 — the same user / movie conditionals, no w draw, w_store may be null).  Prediction
// without side information is the model's a = 1, b = c = 0 with empty feature lists (:1101-1102).
static int cf_gibbs_run(const char* name, const CfModel& M, const CfSchedule& S, const CfFold& fd) {
  std::string err = cf_gibbs_check(name, M, S, fd);
  CfRatings R;
  if (err.empty())
    if (const char* e = cf_split_fold(fd, M, R)) err = e;
  if (!err.empty()) { set_error(err); return GPT_ERR_BAD_DIMS; }
  const CfSizes z = cf_sizes(M, S, std::max(fd.N, fd.Ntest));
  std::vector<double> w0, U0, V0;
  cfg_init(M, S.rotated_w != 0, w0, U0, V0);
  CfFoldDev D; CfGibbsDev G;
  GPT_TRY(D.init(fd, R, z, false, w0.data(), U0.data(), V0.data(), nullptr));
  GPT_TRY(G.init(M, R));
  const CfChain& C = D.C;
  CfSideDev side; CfParams P;
  GPT_TRY(fill_params(M, S, false, side, P));
  DevMem d_ch;
  GPT_HIPCHK(d_ch.upload(&C, 1));
  zero_outputs(fd, z, true, 0.0);
  CfKeep K; StatusRing sr;
  GPT_TRY(K.init(z, fd.Ntest));
  GPT_TRY(sr.init());
  int counter = 0; uint32_t sweep = 0;
  for (int64_t epoch = 1; epoch <= S.burnin + S.maxepoch; ++epoch) {
    for (int64_t g = 0; g < S.n_samples; ++g, ++sweep) {
      const hipError_t e = cfg_sweep(M, C, G, sweep);
      if (e != hipSuccess) return hip_fail(e, name);
    }
    if (epoch > S.burnin) {
      const int64_t s2 = epoch - S.burnin - 1, slot = s2 - K.flushed;
      if (fd.w_store) GPT_HIPCHK(hipMemcpyAsync(K.w + z.rr * slot, C.w, 8 * z.rr, hipMemcpyDeviceToDevice, nullptr));
      GPT_HIPCHK(hipMemcpyAsync(K.U + z.nU * slot, C.U, 8 * z.nU, hipMemcpyDeviceToDevice, nullptr));
      GPT_HIPCHK(hipMemcpyAsync(K.V + z.nV * slot, C.V, 8 * z.nV, hipMemcpyDeviceToDevice, nullptr));
      if (!S.avg) counter = 0;
      hipError_t e = launch_cf_eval(P, d_ch.as<CfChain>(), 1, z.nmax, counter, nullptr);
      if (e == hipSuccess)
        e = launch_cfg_keep(d_ch.as<CfChain>(), (int)fd.Ntest, z.neval, K.rm + 2 * slot,
                            K.tp + (size_t)fd.Ntest * slot, nullptr);
      if (e != hipSuccess) return hip_fail(e, "cf eval kernel");
      counter += 1;
      if (slot + 1 == K.chunkE) GPT_TRY(K.flush(fd, z, C.status, s2 + 1));
    }
    const int ring = (int)(epoch & 1);
    GPT_HIPCHK(hipMemcpyAsync(sr.h + ring, C.status, 4, hipMemcpyDeviceToHost, nullptr));
    GPT_HIPCHK(hipEventRecord(sr.e[ring], nullptr));
    if (epoch > 1) {                        // the previous epoch's status, one epoch behind
      GPT_HIPCHK(hipEventSynchronize(sr.e[ring ^ 1]));
      if (sr.h[ring ^ 1]) {
        GPT_HIPCHK(hipStreamSynchronize(nullptr));
        return cfg_not_spd(fd, z);
      }
    }
  }
  return K.flush(fd, z, C.status, S.maxepoch);
}

extern "C" int gpt_cf_fullw_gibbs(
    const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2, const double* Ratingtest,
    int64_t Ntest, int64_t ldt, double signal_var, double sigma_u, double sigma_w,
    const double* w_init, int64_t r, int64_t burnin, int64_t maxepoch, int64_t n_samples,
    uint64_t seed, double ytrainMean, double ytrainStd, int32_t avg, int32_t rotated_w,
    double* w_store, double* U_store, double* V_store, double* testpred_store, double* trainRMSE,
    double* testRMSE) {
  CfModel M;
  M.n1 = n1; M.n2 = n2; M.r = r; M.signal_var = signal_var; M.sigma_u = sigma_u;
  M.sigma_w = sigma_w; M.w_init = w_init; M.seed = seed;
  CfSchedule S;
  S.burnin = burnin; S.maxepoch = maxepoch; S.avg = avg; S.n_samples = n_samples; S.rotated_w = rotated_w;
  return cf_gibbs_run("GPT_fullw_gibbs", M, S,
                      CfFold{Rating, N, ldr, Ratingtest, Ntest, ldt, ytrainMean, ytrainStd, w_store,
                             U_store, V_store, testpred_store, trainRMSE, testRMSE, GPT_OK});
}

extern "C" int gpt_cf_fixw_gibbs(
    const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2, const double* Ratingtest,
    int64_t Ntest, int64_t ldt, double signal_var, double sigma_u, const double* w, int64_t r,
    int64_t burnin, int64_t maxepoch, int64_t n_samples, uint64_t seed, double ytrainMean,
    double ytrainStd, int32_t avg, int32_t rotated_w, double* U_store, double* V_store,
    double* testpred_store, double* trainRMSE, double* testRMSE) {
  CfModel M;
  M.n1 = n1; M.n2 = n2; M.r = r; M.signal_var = signal_var; M.sigma_u = sigma_u; M.w_init = w;
  M.seed = seed; M.fixw = true;
  CfSchedule S;
  S.burnin = burnin; S.maxepoch = maxepoch; S.avg = avg; S.n_samples = n_samples; S.rotated_w = rotated_w;
  return cf_gibbs_run("GPT_fixw_gibbs", M, S,
                      CfFold{Rating, N, ldr, Ratingtest, Ntest, ldt, ytrainMean, ytrainStd, nullptr,
                             U_store, V_store, testpred_store, trainRMSE, testRMSE, GPT_OK});
}
