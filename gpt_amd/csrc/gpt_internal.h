// Internal declarations shared by the libgptsgld translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "gpt_common.h"
#include "launch_util.h"
#include "../../include/gptsgld.h"

namespace gpt {

#ifndef GPT_NT
#define GPT_NT 512
#endif
#ifndef GPT_WPE
#define GPT_WPE 2
#endif
constexpr int kNT = GPT_NT;        // threads per workgroup (waves of 64)
constexpr int kNW = kNT / 64;      // waves per workgroup
constexpr int kDMax = 16;          // max input dimensions D handled by the kernels
constexpr int kEngineGrid = 0;     // sgld.hip: grid (D+1, chains), two batch reads per step
constexpr int kEngineChain = 1;    // chain.hip: one workgroup per chain, one batch read per step
constexpr int kEngineWave = 3;     // wave.hip: per step a V-phase workgroup per chain, then one
                                   // wave per (chain, dimension) (ranks past the chain engine)
// The store_flags bits of gpt_sgld_session_create (the key closes include/gptsgld.h).
enum SessionFlag : int32_t {
  kFlagStore = 1 << 0,             // keep w_store / U_store
  kFlagDiag = 1 << 1,              // keep the per-step gradient norms
  kFlagGrid = 1 << 2,              // force the grid engine (RMSprop-capable sessions)
  kFlagChain = 1 << 3,             // force the chain engine
  kFlagWonly = 1 << 4,             // GPT_SGLDERMw steps (grid engine)
  kFlagCls = 1 << 5,               // GPTclassification: the chains are the classes (grid engine)
  kFlagSplit = 1 << 6,             // the removed split engine: rejected
  kFlagWave = 1 << 7,              // force the wave engine
};

// Per-chain device state.  All pointers are device pointers.
struct ChainDesc {
  const double* phi;     // n*D*N   training features, Julia layout
  const double* y;       // N       training targets
  int32_t* order;        // 2*N     ring of cumulative epoch orders (0-based rows): order_e at
                         //         (e&1)*N, built on the device (order.hip)
  double* w;             // 2*Q     ping-pong: w_t at (t&1)*Q
  double* U;             // n*r*D   current Stiefel factors (block k owns slice k)
  double* temp;          // 2*D*r*m ping-pong temp[k,l,i] of the NEXT batch
  double* w_store;       // Q*nstore or nullptr
  double* U_store;       // n*r*D*nstore or nullptr
  double* diag;          // (1+D)*steps per-step gradient norms or nullptr
  int32_t* status;       // 0 ok, 1 NaN in geodesic
  uint64_t seed;
  double epsw, epsU, signal_var, sigma_w;   // per-chain hyper-parameters (sweeps)
  double* gw;            // RMSprop (GPT_SGLD.jl:1121): Q moving average of squared gradw
  double* gU;            //   n*r*D moving average of squared gradU
  double* res;           //   m residuals of the step (written by the w phase)
  double* coef;          // wave engine: D*m*r core sums A[l,k,i]*res_i of the step, [(k*m + i)*r + l]
  double* park;          //   n*r*D the Stiefel momentum while the geodesic's expm holds the registers
};

struct StepParams {
  int n, D, N, r, Q, m, nb;       // nb = numbatches = ceil(N/m)
  int burnin_steps;               // burnin*nb
  long long total_steps;
  int store_every;
  int langevin, stiefel;
  const int32_t* I0;              // Q*D 0-based, layout q + Q*k
  const int32_t* runq;            // chain engine: runq[(k*r + l)*64 + s] = s-th q (ascending) with
                                  // I[q,k] = l, or 256 (a zero slot) past the run's end
  const int32_t* vtab;            // grid engine, column-lane V-phase: per workgroup kind (k < D,
                                  // w block = D) and core entry q, 16 ints: 8 temp row offsets
                                  // and I[q, k] (vphase_cols_tables), or null (vphase_tile)
  const uint16_t* wvtab;          // wave engine: V-phase temp offsets, run members, run starts
                                  // (16-bit, wave_tables)
  long long* stamps;              // diagnostic builds: s_memtime per phase per block, else null
  long long* tline;               // chain engine: per-workgroup timeline (kTimeline per block) or null
  int rms;                        // 1: GPT_SGLDERM_RMSprop steps (grid engine, two launches)
  int wonly;                      // 1: GPT_SGLDERMw steps (w alone, U fixed; grid engine)
  int ncls;                       // >= 2: GPTclassification, chains are the classes of one
                                  // model (grid engine; ChainDesc.res = class fhat, .gU = gradU)
  double rms_eps, rms_alpha;      // its epsilon and moving-average coefficient
};
constexpr int kStamps = 16;       // stamp slots per block
constexpr int kTimelineSteps = 512;                 // timeline diagnostics: steps per launch
constexpr int kTimeline = 2 * (kTimelineSteps + 2) + 2;   // int64 per block (+ HW_ID, XCC_ID)
constexpr double kRmsLambda = 1e-5;   // RMSprop smoothing (GPT_SGLD.jl:1146)

GPT_HD size_t al16(size_t x) { return (x + 15) & ~size_t(15); }

// LDS carve of the step kernel (bytes), shared by host (size) and device (offsets).
// Persistent part (whole launch) + a union whose tenants change by phase:
//   V-phase : temp_l                                     (D·R·MP)
//   grads   : W_l | U_l | redG                           (R·NP, R·NP, kNW·max(R²,8))
//   expm    : W_l | expm0 (7·(2R)²) | expm1 (7·R²)       (U_l/redG dead; old U re-read from HBM)
//   update  : W_l | U_l | redG                           (new U; P5 reads U_l)
struct StepLayout {
  int MP, NP, NS, conc, keepU, vcols;   // NP: n padded to 64 (loop range), NS = NP+1 row stride
  size_t o_I, o_w, o_idx, o_y, o_res, o_coef, o_gram, o_Ec, o_mx, o_un;
  size_t o_temp, o_W, o_U, o_red, o_x0, o_x1, o_ones, o_vred, o_vtab, bytes;
};

GPT_HD StepLayout step_layout(int n, int D, int r, int Q, int m) {
  StepLayout L;
  L.MP = ((m + 31) / 32) * 32 + 1;   // odd (bank spread); covers 32-wide unrolled reads
  L.NP = ((n + 63) / 64) * 64;
  L.NS = L.NP + 1;                   // odd stride: rows of U_l/W_l on different banks
  size_t o = 0;
  L.o_I = o;    o = al16(o + 4 * (size_t)Q * D);
  L.o_w = o;    o = al16(o + 8 * (size_t)Q);
  L.o_idx = o;  o = al16(o + 4 * (size_t)m);
  L.o_y = o;    o = al16(o + 8 * (size_t)m);
  L.o_res = o;  o = al16(o + 8 * (size_t)L.MP);
  L.o_coef = o; o = al16(o + 8 * (size_t)r * L.MP);
  L.o_gram = o; o = al16(o + 8 * (size_t)(4 * r * r + r + 2));
  L.o_Ec = o;   o = al16(o + 8 * (size_t)(2 * r * r));
  L.o_mx = o;   o = al16(o + 8 * (size_t)(r * r));
  L.o_un = o;
  const size_t nrp = 8 * (size_t)r * L.NS;
  // Gram scratch: kNW rows of 2r² (blk_gram), padded to the butterfly width of blk_gram_rows
  const int g2 = 2 * r * r, g2p = g2 <= 8 ? 8 : (g2 <= 16 ? 16 : (g2 <= 32 ? 32 : (g2 <= 64 ? 64 : g2)));
  const size_t red = 8 * (size_t)kNW * g2p;
  const size_t x0 = 8 * (size_t)7 * 4 * r * r, x1 = 8 * (size_t)7 * r * r;
  L.o_temp = o;
  L.o_W = o;
  L.o_U = o + nrp;
  L.o_red = L.o_U + nrp;
  const size_t un_v = 8 * (size_t)D * r * L.MP;
  const size_t un_g = 2 * nrp + red;
  size_t un = un_v > un_g ? un_v : un_g;
  const size_t cap = kMaxLds;
  // Preferred: expm scratch after red with U_l kept (old U stays in LDS for tmpU), both expm
  // concurrent.  Fallbacks alias the scratch over U_l/red, then run the two expm in turn.
  if (al16(o + (un > 2 * nrp + red + x0 + x1 ? un : 2 * nrp + red + x0 + x1)) <= cap) {
    L.keepU = 1; L.conc = 1;
    L.o_x0 = L.o_red + red; L.o_x1 = L.o_x0 + x0;
    if (2 * nrp + red + x0 + x1 > un) un = 2 * nrp + red + x0 + x1;
  } else {
    L.keepU = 0;
    L.o_x0 = o + nrp;
    L.conc = (al16(o + (un > nrp + x0 + x1 ? un : nrp + x0 + x1)) <= cap) ? 1 : 0;
    L.o_x1 = L.conc ? L.o_x0 + x0 : L.o_x0;
    const size_t ux = L.conc ? nrp + x0 + x1 : nrp + x0;
    if (ux > un) un = ux;
  }
  // the column-lane V-phase (vphase_cols, D <= 8) keeps after temp_l a row of MP ones, its
  // per-wave partial sums (kNW·(1+r)·64 doubles) and its table (16 ints per q), when that still
  // fits the LDS; otherwise the step uses vphase_tile
  L.o_ones = o + al16(un_v);
  L.o_vred = L.o_ones + al16(8 * (size_t)L.MP);
  L.o_vtab = L.o_vred + 8 * (size_t)kNW * (1 + r) * 64;
  const size_t vend = L.o_vtab + 64 * (size_t)Q - o;
  if (D <= 8 && vend > un && al16(o + vend) <= cap) un = vend;
  L.vcols = (D <= 8 && vend <= un) ? 1 : 0;
  L.bytes = al16(o + un);
  return L;
}

// Host helpers (api_core.hip / api_session.hip / api_pred.hip; sgld.hip, pred.hip)
void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what);
hipError_t set_lds_limits();
size_t pred_lds_bytes(int n, int D, int r, int Q);
bool valid_cfg(const gpt_sgld_config* c);
bool valid_pred(int64_t n, int64_t D, int64_t Ntest, int64_t r, int64_t Q);
bool valid_x_args(const gpt_sgld_config* cfg, int32_t nchains, const uint64_t* seeds,
                  const double* X, const double* const* y, const double* ls, int64_t ls_len,
                  const double* sigma_rbf, const double* Z, const double* b, const int32_t* I,
                  int32_t store_flags);
double host_normal(uint64_t seed, uint32_t e, uint32_t c1, uint32_t c2, uint32_t c3);
void host_stiefel_polar(const double* Z, int r, int n, double* Uk);   // Uk = Zᵀ(ZZᵀ)^(-1/2)
// The session's internals that the host-pointer samplers and classification use next to its C
// entries: chain c's initial state, the per-chain gw | gU | res buffers, and what they read of it.
int session_set_state(gpt_sgld_session* s, int c, const double* w, const double* U);
int session_alloc_aux(gpt_sgld_session* s);
struct SessionRun { long long total_steps, nstore; const double* U0; };   // U0: chain 0's U (device)
SessionRun session_run_info(const gpt_sgld_session* s);

// Launch wrappers implemented in sgld.hip / pred.hip / feature.hip
hipError_t launch_temp_init(const StepParams& P, const ChainDesc* chains, int nchains,
                            const long long* tbase, hipStream_t st);
hipError_t launch_step(const StepParams& P, const ChainDesc* chains, int nchains,
                       const long long* tbase, int t_local, hipStream_t st);
// RMSprop step = w phase (one workgroup per chain) then U phase (D workgroups per chain)
hipError_t launch_step_wonly(const StepParams& P, const ChainDesc* chains, int nchains,
                             const long long* tbase, int t_local, hipStream_t st);
hipError_t launch_step_cls(const StepParams& P, const ChainDesc* chains, int nchains,
                           const long long* tbase, int t_local, hipStream_t st);
hipError_t launch_step_rms(const StepParams& P, const ChainDesc* chains, int nchains,
                           const long long* tbase, int t_local, hipStream_t st);
hipError_t launch_advance(long long* tbase, long long by, hipStream_t st);
// Epoch orders (order.hip): e_fixed >= 0 builds order_{e_fixed}; e_fixed < 0 builds order_{e+1}
// for the epoch e of step tbase[0] + t_local.  ws: epoch_order_ws_ints(N, nchains) ints (0 when
// the shuffle fits LDS).
bool epoch_order_in_lds(int N);
size_t epoch_order_ws_ints(int N, int nchains);
hipError_t launch_epoch_order(const ChainDesc* chains, int nchains, int N, int nb,
                              long long total_steps, const long long* tbase, int t_local,
                              int e_fixed, int32_t* ws, hipStream_t st);
// vphase_cols' tables for a session (step_layout(n, D, r, Q, m).vcols): (D+1)·Q·16 ints
void vphase_cols_tables(const std::vector<int32_t>& I0, int n, int D, int r, int Q, int m,
                        std::vector<int32_t>& out);

// Chain-resident engine (chain.hip): one workgroup per chain, many steps per launch.
bool chain_supported(int n, int D, int r, int Q, int m, bool langevin, bool stiefel,
                     int max_run = 0);
size_t chain_lds_bytes(int n, int D, int r, int Q, int m);
// nsteps consecutive steps per launch (steps t .. t+nsteps-1 of one epoch at most)
hipError_t launch_chain(const StepParams& P, const ChainDesc* chains, int nchains,
                        const long long* tbase, int t_local, int nsteps, hipStream_t st);

// Wave engine (wave.hip): two launches per step (V-phase per chain, then a wave per dimension);
// init = the first step's temp only.
bool wave_supported(int n, int D, int r, int Q, int m, bool langevin, bool stiefel);
void wave_tables(const std::vector<int32_t>& I0, int Q, int D, int r, int m,
                 std::vector<uint16_t>& out);
size_t wv_dim_lds_bytes(int n, int r, int m);
size_t wv_vphase_lds_bytes(int D, int r, int Q, int m);
hipError_t launch_wave(const StepParams& P, const ChainDesc* chains, int nchains,
                       const long long* tbase, int t_local, bool init, hipStream_t st);
hipError_t launch_expm_check(int nn, int count, const double* A, double* E, int32_t* bad, int mode,
                             hipStream_t st, long long* stamps = nullptr);


hipError_t launch_pred_x(const double* w, const double* U, const int32_t* I0, const double* X,
                         const double* ls, const double* Z, const double* bfe, double c, int n,
                         int D, long long Ntest, int r, int Q, int S, double* fhat, hipStream_t st);
size_t pred_x_lds_bytes(int n, int D, int r, int Q);
// Per-phase event timing of the stacked-sample prediction (diagnostics / the benchmark):
// gemm_ms / vphase_ms accumulate over the sample chunks of one call.
struct PredPhaseTiming { double gemm_ms = 0.0, vphase_ms = 0.0; };
int pred_last_vphase();
constexpr int kPredRouteLen = 7;
void pred_last_route(int32_t* out, int len);   // the first len of kPredRouteLen entries
hipError_t launch_pred(const double* w, const double* U, const int32_t* I0, const double* phitest,
                       int n, int D, long long Ntest, int r, int Q, int S, double* fhat,
                       hipStream_t st, PredPhaseTiming* timing = nullptr);
hipError_t pred_trim_pools();      // return the prediction pool's memory (gpt_pred_trim_pool)
hipError_t launch_mean_rmse(const double* fhat, const double* ytest, long long Ntest, int S,
                            double* mean_out, double* sse_out, hipStream_t st);
hipError_t launch_feature(const double* X, long long N, int D, const double* ls, double c,
                          const double* Z, const double* b, int n, double* phi, hipStream_t st);
hipError_t launch_feature_notensor(const double* X, long long N, int D, const double* ls,
                                   double c, const double* Z, const double* b, int n,
                                   double* phi, hipStream_t st);
// X mode (gpt_sgld_session_create_x): the session keeps X, Z, b and per-chain length scales
// instead of an n·D·N phi per chain, and the stager (feature.hip) writes the feature rows of the
// coming minibatches into a per-chain ring of KR batch slots.  The engines run on a second
// ChainDesc array, the engine view: phi = the ring (KR·m rows of n·D doubles), y = a ring of KR·m
// targets, order = a 2·N view laid out like the real order ring whose entry for (epoch e, batch b,
// row i) is the ring row (t mod KR)·m + i, t = e·nb + b.
constexpr int kXSpanCap = 8;      // X mode, chain engine: steps per launch at most
struct StageParams {
  const double* X;                // N*D  training inputs, X[i + N k]
  const double* Z;                // n*D
  const double* b;                // n*D
  const double* ls;               // ls_len*nchains length scales, chain c at ls + ls_len*c
  const double* cfeat;            // nchains: the feature scale c of gpt_feature, per chain
  int ls_len;                     // 1 or D
  int N, n, D, m, nb, KR;
  long long total_steps;
  size_t o_rows;                  // bytes from a chain's feature ring to its KR*m staged row numbers
};
// Stage batches tbase[0] + t_first .. + count - 1 (those below total_steps) of every chain:
// `real` holds the order rings and the targets, `view` the rings written.
hipError_t launch_stage_batches(const StageParams& S, const ChainDesc* real, const ChainDesc* view,
                                int nchains, const long long* tbase, int t_first, int count,
                                hipStream_t st);
// MovieLens tensor CF (cf.hip, 100k_movielensExperiment.jl:409-551)
struct CfParams {
  int n1, D1, n2, D2, r, m, rowsU, rowsV;
  double a, b, c, signal_var, sigma_u, sigma_w, epsw, epsU;
  int langevin, stiefel;
  int fixw;              // GPT_fixw*: w is a fixed argument (no gradw, no w step)
  uint64_t seed;
  const int32_t* uptr;   // n1+1 CSR offsets into ufe: the feature rows (n1 + f) of each user
  const int32_t* ufe;
  const int32_t* vptr;   // n2+1
  const int32_t* vfe;
  const uint64_t* umask;   // n1: bitmask of each user's feature rows (D1 <= 64), else null
  const uint64_t* vmask;   // n2
  long long* stamps;     // diagnostics: kCfStampSteps x kCfStampSlots s_memtime of chain 0, or null
  int exp;               // diagnostic builds only (CF_WSTAMPS): timing experiments, GPTSGLD_CF_EXP
};
// CF_WSTAMPS (diagnostic builds, make diag): 4 more stamps per wave of the 16 (cf.hip CF_WSTAMP)
#ifndef CF_WSTAMPS
#define CF_WSTAMPS 0
#endif
constexpr int kCfStampSteps = 64, kCfStampSlots = CF_WSTAMPS ? 8 + 4 * 16 : 8;

struct CfChain {
  const int32_t* tr_user;   // N   0-based ids
  const int32_t* tr_movie;
  const double* tr_rating;  // N   standardised
  const int32_t* te_user;   // Ntest
  const int32_t* te_movie;
  const double* te_rating;
  int N, Ntest;
  const int32_t* perm;      // N   this epoch's permutation (0-based rows of the ratings)
  int32_t* ep_user;         // N   the training ratings in this epoch's order (cf_gather_kernel)
  int32_t* ep_movie;
  double* ep_rating;
  double* w;                // r*r column-major
  double* U;                // rowsU*r column-major
  double* V;                // rowsV*r
  double* GU;               // rowsU*r zeroed scratch (gradient rows / momentum)
  double* GV;
  double ymean, ystd;       // ytrainMean / ytrainStd of the chain's fold (evaluation)
  double* trainpred;        // N      running averages (avg)
  double* testpred;         // Ntest
  double* sse;              // 2 * gridDim.x partial sums of the eval kernel
  int32_t* status;
};

// How an SGD / SGLD epoch is launched (cf_epoch_kernel's domove; gpt_cf_last_mode reports it):
//   kCfStepPairs     per minibatch a batch-phase launch and a row-parallel cf_move_kernel launch
//   kCfStiefelEpoch  one launch per epoch, the Stiefel move of every row inside it
//   kCfLazyEpoch     one launch per epoch, the lazy SGD move (rows outside a batch only decay)
enum CfMode { kCfStepPairs = 0, kCfStiefelEpoch = 1, kCfLazyEpoch = 2 };

size_t cf_lds_bytes(int r, int m, int nfeat, bool masks);
size_t cf_lazy_lds_bytes(int r, int m, int nfeat, int rows, int nb);
hipError_t launch_cf_epoch(const CfParams& P, const CfChain* chains, int nchains, long long step0,
                           int bt0, int nb, CfMode domove, hipStream_t st,
                           const long long* step_base = nullptr);
hipError_t launch_cf_gather(const CfChain* chains, int nchains, int N, hipStream_t st);
hipError_t launch_cf_move(const CfParams& P, const CfChain* chains, int nchains, long long step,
                          hipStream_t st, const long long* step_base = nullptr);
hipError_t launch_cf_eval(const CfParams& P, const CfChain* chains, int nchains, int nmax,
                          int counter, hipStream_t st);
hipError_t launch_cfg_rows(int side, int r, const double* W, const double* Oth, int rows_oth,
                           double* Me, int rows_me, const int32_t* ptr, const int32_t* lst,
                           const int32_t* other, const double* y, double signal_var, double su2,
                           uint64_t seed, uint32_t sweep, uint32_t stream, int32_t* status,
                           hipStream_t st);
size_t cfg_wsystem_scratch_dbl(int r, int n1);
hipError_t launch_cfg_wsystem(int r, const double* U, int n1, const double* V, int n2,
                              const int32_t* uptr, const int32_t* ulst, const int32_t* movies,
                              const double* y, double alpha, double beta, double ysc,
                              double* scratch, double* M, double* x, hipStream_t st);
hipError_t launch_cfg_keep(const CfChain* chains, int Ntest, int neval, double* rmse,
                           double* tp_out, hipStream_t st);
hipError_t gaussian_draw_prec(double* M, int p, double* x, uint64_t seed, uint32_t c1, uint32_t c2,
                              uint32_t c3, double* z, double* out, int32_t* status, hipStream_t st);
hipError_t gaussian_draw_dense(const double* A, int p, long long N, const double* y, double alpha,
                               double beta, double ysc, uint64_t seed, uint32_t c1, uint32_t c2,
                               uint32_t c3, double* M, double* x, double* z, double* out,
                               int32_t* status, hipStream_t st);
// tgp.hip's dense kernels for other translation units: M = alpha·A·Aᵀ + beta·I (lower 16 × 16
// tiles, fp64 MFMA), out = alpha·A·y, the Cholesky factor in place (blocked for p <= 1024, with Lᵀ
// in the upper triangle) and x := L⁻¹x / L⁻ᵀx against it.
hipError_t dense_syrk(const double* A, int p, long long N, double alpha, double beta, double* M,
                      hipStream_t st);
hipError_t dense_gemv(const double* A, int p, long long N, const double* y, double alpha,
                      double* out, hipStream_t st);
void dense_chol(double* M, int p, int32_t* status, hipStream_t st);
void dense_trsv(const double* M, int p, double* x, int trans, hipStream_t st);
bool gmc_supported(int n, int r);
hipError_t gmc_run(const double* phi, const double* y, const int32_t* I0, int n, int D,
                   long long N, int r, int Q, double signal_var, double epsw, double epsU,
                   int burnin, int maxepoch, int L, uint64_t seed, double* w, double* U,
                   double* w_store, double* U_store, double* accept, int32_t* status,
                   hipStream_t st);
hipError_t tgp_gibbs(const double* b, const double* y, int n, int D, long long N, int r, int q,
                     double sigma, int iters, int burnin, uint64_t seed, const int32_t* I0,
                     double* U, double* W_hist, double* U_hist, int32_t* status, hipStream_t st);
hipError_t launch_gpnt(const double* phi, const double* y, const int32_t* order, int n, int N,
                       int m, int nb, long long total, double signal_var, double sigma_theta,
                       double eps_theta, double decay_rate, uint64_t seed, double* theta,
                       double* theta_store, int32_t* status, const long long* tbase, int t_local,
                       hipStream_t st);

// One chain of the full-theta samplers (gpnt.hip, cls.hip; their frame is theta_chain.h): one
// workgroup per chain, theta (len = n doubles, n*C for the classifier) in LDS for a launch.
struct ThetaChain {
  const int32_t* order;  // epochs*N cumulative epoch orders of the chain's seed (0-based rows)
  double* theta;         // len       current theta
  double* store;         // len*kept
  int32_t* status;       // 0 ok, GPT_ERR_NAN_THETA
  uint64_t seed;
  double eps_theta;
};
struct GpntChain : ThetaChain {   // sibling GPNT_SGLD chains (gpnt.hip)
  double signal_var, sigma_theta;
};
struct GpntLayout {
  int rows, groups;      // rows: feature rows staged per group (0: none); groups per full batch
  size_t o_theta, o_idx, o_y, o_res, o_flag, o_phi, base, bytes;   // base: bytes without the rows
};
GpntLayout gpnt_layout(int n, int N, int m, int rows_cap);   // rows_cap < 0: as many as fit
// steps t0 .. t0+nsteps-1 (0-based, those below total) of every chain
hipError_t launch_gpnt_chain(const double* phi, const double* y, const GpntChain* chains,
                             int nchains, int n, int N, int m, int nb, long long total,
                             double decay_rate, int store_every, long long t0, int nsteps,
                             const GpntLayout& L, hipStream_t st);

// Classification (cls.hip).  GPNT_SGLDclass: a ThetaChain with theta (n x C).
struct NtcChain : ThetaChain {};
struct NtcLayout {
  int CC, stage;         // CC: C rounded up to 2, 4, 8, 16, 32; stage: the batch's phi is in LDS
  size_t o_theta, o_idx, o_yb, o_P, o_flag, o_phi, base, bytes;   // base: bytes without the staged phi
};
NtcLayout ntc_layout(int n, int C, int m);
// steps t0 .. t0+nsteps-1 (0-based, those below total) of every chain; y0: N 0-based labels
hipError_t launch_ntc_chain(const double* phi, const int32_t* y0, const NtcChain* chains,
                            int nchains, int n, int N, int C, int m, int nb, long long total,
                            double decay_rate, int store_every, long long t0, int nsteps,
                            const NtcLayout& L, hipStream_t st);
// scores (Ntest, S) = phitestᵀ (n, Ntest) · theta (n, S)
hipError_t launch_nt_scores(const double* phitest, const double* theta, int n, long long Ntest,
                            long long S, double* scores, hipStream_t st);
// Evaluation of scores (Ntest, C, T) against labels y in 1..C: part_nlp / part_miss hold
// class_eval_tiles(Ntest)*T partial sums; prop_missed, mean_nlp (T); pred_out, nlp_out
// (Ntest*T, optional).
size_t class_eval_tiles(long long Ntest);
hipError_t launch_class_eval(const double* scores, const int32_t* y, long long Ntest, int C, int T,
                             double* part_nlp, int32_t* part_miss, double* prop_missed,
                             double* mean_nlp, int32_t* pred_out, double* nlp_out, hipStream_t st);
hipError_t launch_class_mean(const double* scores, long long Ntest, int C, int first, int last,
                             double* mean_out, hipStream_t st);

// Chain diagnostics (diag.hip) of the window x (P, S, M), sample s of chain m at x + P·s +
// cstride·m, at lags 0 … K <= S − 1: the per-parameter rows (P each), chain_mean / chain_var (P, M),
// acf (P, K + 1) and chain_acf (P, K + 1, M), the last four optional.  ws holds
// diag_ws_doubles(P, M, K) doubles.  The tiling: samples per time chunk, lags per wave and per
// workgroup, and the workgroups along the lags.
int diag_time_chunk();
int diag_lag_block();
int diag_lag_group();
int diag_lag_groups(int K);
size_t diag_ws_doubles(long long P, int M, int K);
hipError_t launch_chain_diag(const double* x, long long P, long long cstride, int S, int M, int K,
                             double* ws, double* mean, double* sd, double* rhat, double* ess,
                             double* mcse, double* tau, int32_t* truncated, double* chain_mean,
                             double* chain_var, double* acf, double* chain_acf, hipStream_t st);

// Posterior predictive of stored predictions F (Ntest, S) against y at noise variance noise_var
// (predictive.hip): fmu, fs2, lp, lpmix (Ntest, each optional); part (2 per tile) and part_cov
// (1 per tile) hold the predictive_tiles(Ntest) partial sums; sums[0..1] = Σ lp, Σ lpmix and
// *covered = the rows inside the 95 % interval, added in tile order.
size_t predictive_tiles(long long Ntest);
hipError_t launch_predictive(const double* F, const double* y, long long Ntest, int S,
                             double noise_var, double* fmu, double* fs2, double* lp, double* lpmix,
                             double* part, int32_t* part_cov, double* sums, double* covered,
                             hipStream_t st);

// Joint likelihood of the full-theta softmax classifier and its gradient (cjoint.hip).
struct CjLayout {
  int CC, TI, theta_lds, nblk;   // CC: C rounded up to 2, 4, 8, 16, 32; TI: data columns per tile;
                                 // theta_lds: theta (n x CC) sits in LDS; nblk: workgroups
  long long ntiles;
  size_t o_sr, o_X, o_inv, o_red, o_phi, o_S, o_theta, bytes;
};
CjLayout cjoint_layout(int n, long long N, int C);
constexpr int kCjMaxBlocks = 256;                 // the bound of the grid-stride over tiles
enum CjMode : int {
  kCjValue = 0,      // the value's partial sums
  kCjTheta = 1,      // and the partials of d/dtheta (the Langevin step)
  kCjFull = 2,       // and those of d/dlength_scale, d/dsigma
  kCjScores = 3,     // scores (N, C) = phi(X)'theta, no likelihood
  kCjFeatures = 4    // diagnostics: the tile's phi and S only (the sincos share of an evaluation)
};
struct CjArgs {
  const double* X;         // N*D   rows to evaluate, X[i + N k]
  long long N;
  int D, n, C;
  const int32_t* y0;       // N     0-based labels (unused by kCjScores / kCjFeatures)
  const double* Z;         // n*D
  const double* b;         // n
  const double* ls;        // D     length scales
  double c;                // sqrt(2/n)·sigma_RBF
  const double* theta;     // n*C
  double* part_theta;      // nblk*n*C  per-workgroup partials of phi·R'
  double* part_tx;         // nblk*D*n  per-workgroup partials of (S o theta R)·X, [k][j]
  double* part_sc;         // nblk*2    per-workgroup value and sigma sums
  double* scores;          // N*C       (kCjScores)
  const int32_t* status;   // non-zero: the launch does nothing (a Langevin run that met a NaN)
};
hipError_t launch_cjoint_eval(const CjArgs& A, const CjLayout& L, int mode, hipStream_t st);
// out = [value; d/dsigma; d/dl (D); d/dtheta (n*C)], the last two blocks only with `full`
hipError_t launch_cjoint_finish(const CjArgs& A, const CjLayout& L, double sigma, bool full,
                                double* out, hipStream_t st);
// theta <- theta - (eps/2·(sum of the partials + theta) + sqrt(eps)·xi), xi of 0-based step t
hipError_t launch_cjoint_update(const CjArgs& A, const CjLayout& L, double* theta, double eps,
                                uint64_t seed, uint32_t t, int32_t* status, hipStream_t st);

// Hamiltonian Monte Carlo on the resident theta of the joint likelihood (chmc.hip).
// Entry e = c*n + j of an n*C array belongs to thread e of a grid of hmc_blocks(n, C) workgroups.
constexpr int kHmcMaxBlocks = (1024 * 32 + kNT - 1) / kNT;
int hmc_blocks(int n, int C);
struct HmcDev {
  double* theta;           // n*C   the chain's state (the evaluator's resident theta)
  double *q, *p;           // n*C   work position and momentum
  double *g_cur, *g_new;   // n*C   grad U at theta (the cache) and at the last evaluation's q
  double *kin0, *kin1;     // hmc_blocks  per-workgroup sums of p^2 at the start and the end
  double* prior;           // hmc_blocks  per-workgroup sums of q^2 at the last evaluation's q
  double* sc;              // 4     [0] U(theta) (the cache), [2] H0 and [3] H1 of the integrator alone
  int32_t* flag;           // 1     the last decision: 1 accepted
  long long* ndiv;         // 1     divergent transitions of the call
  const int32_t* status;   // non-zero: every launch does nothing
  int n, C;
};
// p of transition t (draw: element j of the normal stream (seed, t, kHmcMom, c); otherwise the p
// in place), q <- theta, kin0
hipError_t launch_hmc_begin(const HmcDev& S, bool draw, uint64_t seed, uint32_t t, hipStream_t st);
// kind 0: p -= s/2 g_cur, q += s p; 1: g = sum of the partials + q, p -= s g, q += s p;
// 2: p -= s/2 g, g_new = g, kin1 and prior.  s = sqrt(eps).
hipError_t launch_hmc_leap(const HmcDev& S, int kind, const double* part_theta, int nblk, double s,
                           hipStream_t st);
// after an evaluation at theta: g_cur and prior
hipError_t launch_hmc_prime(const HmcDev& S, const double* part_theta, int nblk, hipStream_t st);
// mode 0: sc[0] = U(theta); 1: the Metropolis decision of transition t, record i of the call;
// 2: sc[2], sc[3] = H0, H1
hipError_t launch_hmc_decide(const HmcDev& S, int mode, const double* part_sc, int nblk,
                             uint64_t seed, uint32_t t, long long i, int32_t* acc_rec,
                             double* dh_rec, double* val_rec, hipStream_t st);
// theta <- q, g_cur <- g_new where accepted; store_col (n*C or null) <- the kept theta
hipError_t launch_hmc_commit(const HmcDev& S, double* store_col, hipStream_t st);

// Host-side Philox consumers (init / permutations / samplenz)
void host_init_state(int n, int r, int D, int Q, uint64_t seed, bool stiefel, double sigma_w,
                     double* w, double* U, int cls = 0, bool cls_init = false);
void host_epoch_orders(int N, uint64_t seed, int epochs, int32_t* out);  // E*N cumulative

}  // namespace gpt
