/* gptsgld.h — C ABI of libgptsgld.so, the MI355X-native tensor-GP SGLD path.
 *
 * Drop-in boundary for the Julia module API that the reference's experiment scripts import
 * with `@everywhere using GPT_SGLD` (kin40kExperiment.jl:3).  Each entry point below names
 * the reference function it replaces (file:line under hyunjik11/GPT).  INTEGRATION.md shows
 * the Julia `ccall` shim and the Python ctypes binding.
 *
 * Conventions:
 *  - Arrays are Julia column-major: phi[j,k,i] at j + n*(k + D*i); U[j,l,k] at j + n*(l + r*k);
 *    I[q,k] (Int32, 1-based, values 1..r) at q + Q*k; X[i,k] at i + N*k; Float64 everywhere.
 *  - The caller allocates every output (zero-copy with `ccall(..., Ptr{Float64})`).  The
 *    library owns only device scratch.
 *  - Return value: GPT_OK, or an error code; gpt_last_error() has a thread-local message.
 *    GPT_ERR_NAN_GEODESIC mirrors GPT_SGLD.jl:23-26,422-424: the sample stores are zero-filled.
 *  - Host-pointer entry points copy to the device, run, and copy back (PCIe included).
 *    The *_dev entry points take device pointers and a hipStream_t (as void*) and are what the
 *    benchmark times (inputs resident in HBM).
 *  - Reentrant: no global state except the per-thread error string.
 */
#ifndef GPTSGLD_H
#define GPTSGLD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPT_OK 0
#define GPT_ERR_NAN_GEODESIC 1
#define GPT_ERR_BAD_DIMS 2
#define GPT_ERR_HIP 3
#define GPT_ERR_NAN_THETA 4
#define GPT_ERR_NOT_SPD 5      /* a Gibbs precision matrix failed Cholesky (PosDefException) */

/* Sampler configuration: the scalar arguments of GPTregression (GPT_SGLD.jl:345) plus the
 * framework's store policy.  sigma_w = 1 is Generation C/D (GPT_SGLD.jl:354); Generation A/B
 * (GPT_SGLDERM, GPT_SGLD_p.jl:155) passes sigma_w = sqrt(n^D/Q) and signal_var = sigma^2. */
typedef struct gpt_sgld_config {
  int64_t n;          /* random features per input dimension (reference `n`)            */
  int64_t D;          /* input dimensions                                               */
  int64_t N;          /* training rows                                                  */
  int64_t r;          /* Stiefel rank                                                   */
  int64_t Q;          /* non-zeros of the sparse Tucker core                            */
  int64_t m;          /* minibatch size (reference `m`)                                 */
  double epsw, epsU;  /* SGLD step sizes                                                */
  double signal_var;  /* observation noise variance                                     */
  double sigma_w;     /* prior s.d. of w                                                */
  int64_t burnin, maxepoch;
  uint64_t seed;      /* param_seed: Philox key of every draw of this chain             */
  int32_t langevin;   /* 1 = SGLD (noise), 0 = SGD                                      */
  int32_t stiefel;    /* 1 = geodesic Stiefel update, 0 = Euclidean update of U         */
  int64_t store_every;/* 1 = reference (every post-burn-in step); numbatches = epoch ends */
  int64_t max_steps;  /* 0 = run all (burnin+maxepoch)*numbatches steps                  */
} gpt_sgld_config;

/* ---- features ------------------------------------------------------------------------ */
/* feature(X,length_scale,sigma_RBF,phi_scale,Z,b)  GPT_SGLD.jl:71-84  -> phi (n,D,N) */
int gpt_feature(const double* X, int64_t N, int64_t D, const double* length_scale,
                int64_t ls_len, double sigma_rbf, double phi_scale, const double* Z,
                const double* b, int64_t n, double* phi_out);
/* featureNotensor(X,length_scale,sigma_RBF,Z,b)  GPT_SGLD.jl:109-120  -> phi (n,N) */
int gpt_feature_notensor(const double* X, int64_t N, int64_t D, const double* length_scale,
                         int64_t ls_len, double sigma_rbf, const double* Z, const double* b,
                         int64_t n, double* phi_out);
/* Device form of gpt_feature (all pointers device, hip_stream may be NULL). */
int gpt_feature_dev(const double* X_dev, int64_t N, int64_t D, const double* ls_dev,
                    int64_t ls_len, double sigma_rbf, double phi_scale, const double* Z_dev,
                    const double* b_dev, int64_t n, double* phi_dev, void* hip_stream);
/* seeded Generation-C inputs of feature(X,n,ls,σ,seed,scale): Z=randn(n,D), b=2π·rand(n,D) */
int gpt_feature_inputs(int64_t n, int64_t D, uint64_t seed, double* Z_out, double* b_out);
/* seeded Generation-A inputs of feature(X,n,length_scale,seed)  GPT_SGLD_p.jl:40-54:
 * Z = randn(n,D) (the Gen-C Z stream), b = randn(n,D) (its own stream); the caller applies
 * Z/length_scale and scale sqrt(2/n) with sigma = 1 (gpt_feature with phi_scale = 1). */
int gpt_feature_inputs_a(int64_t n, int64_t D, uint64_t seed, double* Z_out, double* b_out);

/* samplenz(r,D,Q,seed)  GPT_SGLD.jl:181-190 / GPT_SGLD_p.jl:57-67  -> I (Q,D) Int32 1-based */
int gpt_samplenz(int64_t r, int64_t D, int64_t Q, uint64_t seed, int32_t* I_out);

/* Initial state of GPTregression (GPT_SGLD.jl:357-369): w (Q), U (n,r,D). */
int gpt_sgld_init(const gpt_sgld_config* cfg, double* w_out, double* U_out);

/* ---- sampler ------------------------------------------------------------------------- */
/* GPTregression(phi,y,signal_var,I,r,Q,m,epsw,epsU,burnin,maxepoch,param_seed;langevin,stiefel)
 * GPT_SGLD.jl:345-448 (also GPT_SGLDERM, GPT_SGLD_p.jl:146-243, via sigma_w/signal_var).
 * w_init/U_init: NULL = draw from the seed (the reference's srand(param_seed) path).  With
 * stiefel, U_init must have orthonormal columns per dimension (as the reference's init does): the
 * geodesic takes Uᵀmom as (M − Mᵀ)/2 from the projection's M = UᵀW, which holds on the manifold.
 * w_store (Q,T), U_store (n,r,D,T) with T = maxepoch*numbatches/store_every.
 * diag (nullable): per step [‖gradw‖, ‖gradU_1‖ … ‖gradU_D‖] ((1+D) x steps). */
int gpt_sgld_regression(const gpt_sgld_config* cfg, const double* phi, const double* y,
                        const int32_t* I, const double* w_init, const double* U_init,
                        double* w_store, double* U_store, double* diag);

/* Independent GPTregression chains in one call, from host arrays (kin40kExperiment.jl:67-74: the
 * `@parallel for j=1:10` sweep block, every sweep its own phi from its own length scales and
 * sigma_RBF; or posterior chains sharing one phi, BASELINE config 4).  It builds a device session
 * internally, so the multi-chain engines (chain engine r <= 5, wave engine r = 6..20; the grid
 * engine while nchains·(D+1) workgroups fit the CUs; GPTSGLD_ENGINE overrides) serve a host that
 * has no device memory of its own (the Julia shim).  phi[c] (n,D,N), y[c] (N): chain c's inputs
 * (pointers may repeat; each distinct array is copied to the device once).  seeds[c]: param_seed.
 * epsw / epsU / signal_var: NULL = cfg's value for every chain, else one per chain (sigma_w is
 * cfg's).  w_store[c] (Q,T), U_store[c] (n,r,D,T), T = maxepoch*numbatches/store_every, as
 * gpt_sgld_regression (both NULL: no stores).  status[c]: GPT_OK, or GPT_ERR_NAN_GEODESIC with
 * that chain's stores zero-filled (GPT_SGLD.jl:422-424); the return value is GPT_OK when every
 * chain ran to its end or bailed out. */
int gpt_sgld_regression_chains(const gpt_sgld_config* cfg, int32_t nchains, const uint64_t* seeds,
                               const double* const* phi, const double* const* y, const int32_t* I,
                               const double* epsw, const double* epsU, const double* signal_var,
                               double* const* w_store, double* const* U_store, int32_t* status);

/* gpt_sgld_regression_chains from X (kin40kExperiment.jl:67-74: every sweep's phitrain is
 * feature(Xtrain, n, length_scale_j, sigma_RBF_j, seed, scale) of the same Xtrain, Z and b): chain
 * c's features are formed on the device, minibatch by minibatch, from X (N,D), Z (n,D), b (n,D)
 * (shared), length_scale (ls_len, nchains) with ls_len 1 or D, sigma_rbf (nchains) and phi_scale,
 * so no phi (n,D,N) is computed, held or copied: the same doubles gpt_feature makes, hence the
 * same stores as gpt_sgld_regression_chains on feature(X, length_scale[:,c], sigma_rbf[c], ...).
 * y[c], seeds, epsw / epsU / signal_var, w_store, U_store and status as there.  Each distinct
 * host array is copied to the device once; every argument is checked before the first device
 * call. */
int gpt_sgld_regression_chains_x(const gpt_sgld_config* cfg, int32_t nchains, const uint64_t* seeds,
                                 const double* X, const double* const* y,
                                 const double* length_scale, int64_t ls_len,
                                 const double* sigma_rbf, double phi_scale, const double* Z,
                                 const double* b, const int32_t* I, const double* epsw,
                                 const double* epsU, const double* signal_var,
                                 double* const* w_store, double* const* U_store, int32_t* status);

/* GPT_SGLDERM_RMSprop(phi,y,signal_var,I,r,Q,m,epsilon,alpha,burnin,maxepoch)
 * GPT_SGLD.jl:1121-1237: per-entry RMSprop step sizes for w, one averaged step per U^(k), w
 * updated before A.  cfg's epsw/epsU/sigma_w are not used (sigma_w = 1 as in the reference);
 * cfg->langevin and cfg->stiefel must be 1.  Runs on the grid engine. */
/* GPT_SGLDERMw(phi,y,signal_var,I,r,Q,m,epsw,burnin,maxepoch)  GPT_SGLD.jl:1065-1118: SGLD on w
 * alone, U fixed at its uniform Stiefel draw (cfg: stiefel = langevin = 1, sigma_w = 1; epsU is
 * unused).  w_store (Q, maxepoch*numbatches), U_out (n, r, D) = the fixed U, diag row 0 = |gradw|
 * per step.  Runs on the grid engine (store_flags bit 4 in a session). */
int gpt_sgld_wonly(const gpt_sgld_config* cfg, const double* phi, const double* y, const int32_t* I,
                   const double* w_init, const double* U_init, double* w_store, double* U_out,
                   double* diag);
/* GPTclassification(phi,y,I,r,Q,m,epsw,epsU,burnin,maxepoch,param_seed;langevin,stiefel)
 * GPT_SGLD.jl:452-680: softmax tensor-GP classifier; y holds labels 1..C (as doubles).  cfg:
 * signal_var / sigma_w are not used (the model has no noise variance, sigma_w = 1).  Optional
 * w_init (Q, C) / U_init (n, r, D, C).  w_store (Q, C, maxepoch*numbatches), U_store
 * (n, r, D, C, ...); diag (1+D, steps, C) per-class gradient norms.  As the reference, w and U
 * move twice per step with one gradient (an SGLD + Stiefel move, then the langevin/stiefel
 * variant).  Grid engine (store_flags bit 5 in a session: the chains are the C classes). */
int gpt_sgld_classification(const gpt_sgld_config* cfg, const double* phi, const double* y,
                            const int32_t* I, const double* w_init, const double* U_init,
                            double* w_store, double* U_store, double* diag);
int gpt_sgld_rmsprop(const gpt_sgld_config* cfg, double epsilon, double alpha, const double* phi,
                     const double* y, const int32_t* I, const double* w_init,
                     const double* U_init, double* w_store, double* U_store, double* diag);

/* Multi-chain, device-resident session (benchmark / multi-GPU path).  Chains share the
 * config except seed; chain c reads phi_dev[c], y_dev[c] (device pointers; may alias). */
typedef struct gpt_sgld_session gpt_sgld_session;
int gpt_sgld_session_create(const gpt_sgld_config* cfg, int32_t nchains, const uint64_t* seeds,
                            const double* const* phi_dev, const double* const* y_dev,
                            const int32_t* I_host, int32_t store_on_device, void* hip_stream,
                            gpt_sgld_session** out);
/* X mode: a session that trains from X (the sweep block of kin40kExperiment.jl:67-74, where the
 * sweeps' phi differ only in length_scale and sigma_RBF).  It holds X_dev (N,D), Z_dev, b_dev
 * (n,D) (device, column-major, shared by the chains), ls_dev (ls_len, nchains) (device; ls_len 1
 * or D) and sigma_rbf (host, nchains), and never an n*D*N phi: before the steps that read them, a
 * kernel writes the feature rows of the coming minibatches into a ring of a few batch slots per
 * chain (gpt_sgld_session_staging), as the doubles gpt_feature_dev makes, and the step engines
 * read the ring.  store_flags: bits 0, 1 (stores, diagnostics) and the engine bits 2, 3, 7; the
 * RMSprop, w-only and classification steps and the stamps / timeline diagnostics are
 * GPT_ERR_BAD_DIMS on an X session; every other session call works as for a phi session.  The
 * arguments are checked before the first device call. */
int gpt_sgld_session_create_x(const gpt_sgld_config* cfg, int32_t nchains, const uint64_t* seeds,
                              const double* X_dev, const double* const* y_dev,
                              const double* ls_dev, int64_t ls_len, const double* sigma_rbf,
                              double phi_scale, const double* Z_dev, const double* b_dev,
                              const int32_t* I_host, int32_t store_flags, void* hip_stream,
                              gpt_sgld_session** out);
/* out[3] = {batch slots KR of a chain's ring, staging bytes per chain = KR*m*(8*n*D + 8 + 4) for
 * the feature rows, targets and row numbers + 4*2*N for the order view, 1 for an X session};
 * {0, 0, 0} for a phi session.  KR = the steps of one launch + 1 (2 on the grid and wave engines,
 * 9 on the chain engine, whose X-mode launches run 8 steps at most), whatever N. */
int gpt_sgld_session_staging(gpt_sgld_session* s, int64_t* out);
/* Per-chain step sizes / variances (a hyper-parameter sweep, kin40kExperiment.jl:67-74);
 * call before the first run. */
int gpt_sgld_session_set_hyper(gpt_sgld_session* s, int32_t chain, double epsw, double epsU,
                               double signal_var, double sigma_w);
/* Queue `nsteps` SGLD steps of every chain on the session stream (asynchronous).  Whole epochs
 * replay one captured hipGraph; partial chunks replay a graph when one was prepared for them. */
int gpt_sgld_session_run(gpt_sgld_session* s, int64_t nsteps);
/* Capture (without running) the graphs a following gpt_sgld_session_run(s, nsteps) will replay,
 * so that run launches no individual kernels and pays no capture inside a timed region. */
int gpt_sgld_session_prepare(gpt_sgld_session* s, int64_t nsteps);
/* Switch a grid-engine session (store_flags bit 2) to GPT_SGLDERM_RMSprop steps; call before
 * the first run. */
int gpt_sgld_session_set_rmsprop(gpt_sgld_session* s, double epsilon, double alpha);
int gpt_sgld_session_sync(gpt_sgld_session* s);
/* Device pointers of chain c's current state and stores (for pred / collectives). */
int gpt_sgld_session_state(gpt_sgld_session* s, int32_t chain, double** w_dev, double** U_dev,
                           double** w_store_dev, double** U_store_dev, int64_t* nstore);
/* Current state of chains first .. first+count-1 packed on the device for stacked-sample
 * prediction (gpt_pred_dev with S = count): w_dev_out (Q, count), U_dev_out (n*r*D, count).
 * Ordered on the session stream. */
int gpt_sgld_session_gather_state(gpt_sgld_session* s, int32_t first, int32_t count,
                                  double* w_dev_out, double* U_dev_out);
int64_t gpt_sgld_session_steps_done(gpt_sgld_session* s);
/* Run `nsteps` steps WITHOUT graph capture, bracketing every step-kernel launch with hipEvents;
 * *avg_us = mean step-kernel duration (the roofline's per-launch time).  Synchronises. */
int gpt_sgld_session_time_steps(gpt_sgld_session* s, int64_t nsteps, double* avg_us);
/* Diagnostic: run nsteps un-captured steps recording s_memtime (shader-clock ticks)
 * stamps per phase; out = nsteps x W x 16 int64 (0 = phase not reached), W = the workgroups of
 * one step ((D+1)*nchains, grid engine; gpt_sgld_session_info). */
int gpt_sgld_session_stamps(gpt_sgld_session* s, int64_t nsteps, int64_t* out);
/* Diagnostic (chain engine): ONE launch of nsteps steps (within the current epoch, <= 512);
 * out = nchains x gpt_sgld_timeline_slots() int64: per block {s_memrealtime, s_memtime} at slot
 * 0 = entry, 1 = prologue end and 2 + s = end of step s, then HW_ID and XCC_ID.  The product
 * library fills slots 0, 1 and the last step's; the timeline build (`make timeline`) every step.
 * *event_us = the launch's hipEvent time. */
int64_t gpt_sgld_timeline_slots(void);
/* Test entry: E = expm(A) for `count` row-major nn x nn host matrices on the device, at every size
 * the samplers instantiate (the geodesic's 2r x 2r block and the r x r expm(-tA)):
 *   mode 0  the wave engine's register-blocked Padé (wave.hip wv_expm), every column;
 *           nn in {6,8,10,12,15,16,20,24,30,32,40}
 *   mode 1  wave_expm of the grid, chain, TGP and MovieLens kernels;
 *           nn in {1,2,3,4,5,6,8,10,12,15,16,20,24,30,32,40}
 *   mode 3  wave_expm with the LDS partial-pivoting solve kept (the 1024-thread kernels); nn = 40
 *   mode 4  wv_expm asked for the first nn/2 result columns only, as the wave engine's geodesic
 *           calls it; E_c is the whole result slot, of which columns [0, nn/2) are defined;
 *           nn in {12,16,20,24,30,32,40}
 *   mode 5  wave_expm with the degree 3..9 polynomial kept in its LDS form, at the sizes where
 *           mode 1 runs it register-resident (the two must agree bitwise); nn in {1,2,3,4,5,6,8,10}
 * (mode 2 is gpt_debug_expm_stamps' timing run.)  Any other (mode, nn) is GPT_ERR_BAD_DIMS.
 * bad[c] = 1 when E_c holds a NaN (the geodesic bail-out test); for an A_c with an Inf or NaN
 * entry bad[c] = 1 and E_c is all NaN. */
int gpt_debug_expm(int32_t nn, int32_t count, int32_t mode, const double* A, double* E,
                   int32_t* bad);
/* Test entry: the Gaussian conditional draw of the Gibbs samplers (tgp.hip gaussian_draw_prec,
 * GPT_fullw_gibbs w | U, V at 100k_movielensExperiment.jl:1092-1094, TGP.jl:61-63): M (p × p,
 * column-major, SPD; its lower triangle is read) = L·Lᵀ, out = L⁻ᵀz + M⁻¹x with z the Philox
 * normals (seed, c1, c2, c3) of element e = 0..p-1; *status = 1 if M is not positive definite. */
int gpt_debug_gaussian_draw(int32_t p, const double* M, const double* x, uint64_t seed, uint32_t c1,
                            uint32_t c2, uint32_t c3, double* out, int32_t* status);
/* Test entry: the initial U ((n1+D1) x r) and V ((n2+D2) x r), both column-major, of the next CF
 * SGD / SGLD run on this thread (gpt_cf_fullw_sideinfo, gpt_cf_fixw_sideinfo, gpt_cf_fullw,
 * gpt_cf_fixw, gpt_cf_fullw_sideinfo_folds: every fold starts from them) in place of the host's
 * Philox draw.  The arrays are copied.  One shot: that run takes the pair and clears it whether or
 * not it succeeds; rows or rank that differ from the run's are GPT_ERR_BAD_DIMS there, with a
 * message.  The Stiefel path takes the columns as they are (orthonormal is the caller's business).
 * U0 = V0 = NULL clears a pending pair; one of them NULL, rows < 1 or r < 1 is GPT_ERR_BAD_DIMS. */
int gpt_debug_cf_init(const double* U0, int64_t rowsU, const double* V0, int64_t rowsV, int64_t r);
/* Test entry: one function of the noise path (gpt_amd/csrc/fastmath.h, gpt_common.h) evaluated on
 * the device on `count` host inputs, called as the engines call it (coefficients through the
 * constant table, the sin/cos tables filled in LDS by sincos_tab_fill).  fn:
 *   0  fm_log_c(x[i]) -> out0                   5  the 64 doubles of the filled LDS table -> out0
 *   1  fm_sqrt_pos(x[i]) -> out0                   (count must be 64; no input)
 *   2  fm_rcp(x[i]) -> out0                     6  u53(xi[2i], xi[2i+1]) -> out0
 *   3  fm_sincos_2pi_c(x[i]) -> sin out0,       7  u32u(xi[i]) -> out0
 *      cos out1                                 8  fm_sqrt_pos(-2 fm_log_c(x[i])) -> out0, the
 *   4  fm_sincos_tab2(xi[i]) -> sin out0,          Box–Muller radius as the generators form it
 *      cos out1
 * x is read by fn 0-3 and 8, xi by fn 4, 6 and 7, out1 is written by fn 3 and 4; the others may be
 * null.  An unknown fn, count < 1 or > 2^24, or a missing array is GPT_ERR_BAD_DIMS. */
int gpt_debug_fastmath(int32_t fn, int64_t count, const double* x, const uint32_t* xi, double* out0,
                       double* out1);
/* Test entry: Philox blocks c0 = c0_first .. c0_first + nblocks - 1 of stream (c1, c2, c3) under
 * `seed` on the device: words[4b .. 4b+3] = the four raw Philox words of block b, and z = the
 * normals generator `gen` makes of each block:
 *   0  normal_at, elements 2 c0 and 2 c0 + 1      -> z[2b], z[2b+1]   (c0_first + nblocks <= 2^31:
 *                                                     the element index is a 32-bit word)
 *   1  normal_pair                                -> z[2b], z[2b+1]
 *   2  normal_quad<4>                             -> z[4b .. 4b+3]
 *   3  normal_quad<2> (the first pair)            -> z[2b], z[2b+1]
 *   4  normal_quad_tab<4>                         -> z[4b .. 4b+3]
 *   5  normal_quad_tab<2>                         -> z[2b], z[2b+1]
 *   6  no device work: the host's philox4x32 words, and z[2b], z[2b+1] = the host's u53 of words
 *      (0, 1) and (2, 3)
 * c0_first + nblocks may reach 2^32 (gen 1-6).  An unknown gen, nblocks < 1 or > 2^24, a block
 * range past the top, or a null array is GPT_ERR_BAD_DIMS. */
int gpt_debug_normals(int32_t gen, uint64_t seed, uint32_t c0_first, int64_t nblocks, uint32_t c1,
                      uint32_t c2, uint32_t c3, double* z, uint32_t* words);
/* Timing of the wave engine's expm as geod calls it (three LDS slots, the first nn/2 result
 * columns), one wave per matrix: stamps[4·m + 0..3] = s_memtime at entry, after the Padé
 * polynomial, after the solve, at exit (diagnostics; scripts/expm_bench.py). */
int gpt_debug_expm_stamps(int32_t nn, int32_t count, const double* A, int64_t* stamps);
int gpt_sgld_session_timeline(gpt_sgld_session* s, int64_t nsteps, int64_t* out, double* event_us);
/* Copy chain c's stores / status back (status: GPT_OK or GPT_ERR_NAN_GEODESIC; stores are
 * zero-filled for a non-zero status). */
int gpt_sgld_session_fetch(gpt_sgld_session* s, int32_t chain, double* w_store, double* U_store,
                           double* diag, int32_t* status);
void gpt_sgld_session_destroy(gpt_sgld_session* s);
/* out[4] = {engine, LDS bytes per workgroup, threads per workgroup, workgroups per step launch}.
 * Engines: 0 grid (sgld.hip: D+1 workgroups per chain, one step per launch), 1 chain (chain.hip:
 * one workgroup per chain, up to an epoch of steps per launch; r <= 5), 3 wave (wave.hip: per
 * step a V-phase workgroup per chain, then one wave per (chain, dimension); the figures are the
 * dimension launch's).  Engine 2 (the round-3 split engine) was removed.
 * store_flags of gpt_sgld_session_create: bit0 stores, bit1 diagnostics, bit2 force the grid
 * engine, bit3 force the chain engine, bit7 force the wave engine (bit6, the split engine, is
 * rejected).  Default: the chain engine whenever the shape allows it (few chains: the grid engine
 * while nchains*(D+1) workgroups fit the GPU's CUs), else the wave engine whenever the shape
 * allows it (SGLD + Stiefel, r in {6,8,10,12,15,16,20}, 3r <= n <= 256, m <= 64), else the grid
 * engine; GPTSGLD_ENGINE=grid|chain|wave overrides the default. */
int gpt_sgld_session_info(gpt_sgld_session* s, int64_t* out);

/* ---- prediction ---------------------------------------------------------------------- */
/* pred(w,U,I,phitest)  GPT_SGLD.jl:233-243  -> fhat (Ntest) */
int gpt_pred(const double* w, const double* U, const int32_t* I, const double* phitest,
             int64_t n, int64_t D, int64_t Ntest, int64_t r, int64_t Q, double* fhat_out);
/* Device form over S stored samples: fhat_dev (Ntest,S) = pred of each sample.
 * I_dev is 0-based Int32 (Q,D). */
int gpt_pred_dev(const double* w_dev, const double* U_dev, const int32_t* I0_dev,
                 const double* phitest_dev, int64_t n, int64_t D, int64_t Ntest, int64_t r,
                 int64_t Q, int64_t S, double* fhat_dev, void* hip_stream);
/* The stacked-sample prediction keeps its pass buffers (up to 8 GiB) in a private stream-ordered
 * pool between calls; this returns that memory to the device. */
int gpt_pred_trim_pool(void);
/* gpt_pred_dev with per-phase event timing (diagnostics / the benchmark): ms_out[0] = the
 * phidotU GEMM (fp64 MFMA) kernels, ms_out[1] = the V-phase kernels, summed over the sample
 * chunks of the call; synchronises hip_stream. */
int gpt_pred_dev_timed(const double* w_dev, const double* U_dev, const int32_t* I0_dev,
                       const double* phitest_dev, int64_t n, int64_t D, int64_t Ntest, int64_t r,
                       int64_t Q, int64_t S, double* fhat_dev, void* hip_stream, double* ms_out);
/* The V-phase kernel the last gpt_pred* call on this thread launched (measurement, no reference
 * counterpart): 0 pred_vphase_pairs_kernel, 1 pred_vphase_rows_pf_kernel, 2 pred_vphase_rows_kernel,
 * 4 pred_kernel (the direct path, no separate V-phase); -1 before any call. */
int gpt_pred_last_vphase(int32_t* kind);
/* The route of the last gpt_pred* call on this thread (measurement, for the route assertions of
 * tests/test_gpu_pred.py); the first min(len, 7) of: [0] the kind of gpt_pred_last_vphase, [1] the
 * kernel's template dimension (NT of the pair-table kernel, DD of the persistent rows kernel with
 * 0 = run-time D, else 0), [2] its prefetched rows per wave (else 0), [3] the V-phase grid.x and
 * [4] the (sample, 64-row) tiles of the last pass, [5] the passes, [6] the samples in the first
 * pass.  Entries past 7 are set to 0.  GPTSGLD_PRED_PASS_BYTES=<bytes> (read on every call) replaces
 * the 8 GiB temp budget of a pass, never below one sample. */
int gpt_pred_last_route(int32_t* out, int32_t len);
/* Posterior-mean prediction over S samples + RMSE (GPT_SGLD_p.jl:124-132,
 * kin40kExperiment.jl:80-87): mean_out (Ntest), returns rmse*scale in *rmse_out. */
int gpt_pred_mean(const double* w_store, const double* U_store, const int32_t* I,
                  const double* phitest, const double* ytest, int64_t n, int64_t D,
                  int64_t Ntest, int64_t r, int64_t Q, int64_t S, double scale,
                  double* mean_out, double* rmse_out);

/* Fused feature + posterior-mean prediction (§8(f) per-epoch evaluation, kin40kExperiment.jl:78-87):
 * the test features phi = feature(Xtest, length_scale, sigma_rbf, phi_scale, Z, b) are formed
 * inside the prediction kernel (no n*D*Ntest phitest array; the same doubles gpt_feature makes).
 * Xtest (Ntest, D) column-major.  mean_out (Ntest) and *rmse_out as gpt_pred_mean;
 * sample_rmse_out (S, optional) = scale*||ytest - pred(sample s)||/sqrt(Ntest), the testRMSE curve. */
int gpt_pred_mean_x(const double* w_store, const double* U_store, const int32_t* I,
                    const double* Xtest, const double* ytest, int64_t Ntest, int64_t D,
                    const double* length_scale, int64_t ls_len, double sigma_rbf, double phi_scale,
                    const double* Z, const double* b, int64_t n, int64_t r, int64_t Q, int64_t S,
                    double scale, double* mean_out, double* rmse_out, double* sample_rmse_out);

/* ---- full-theta model (config 1) ----------------------------------------------------- */
/* GPNT_SGLD(phi,y,signal_var,sigma_theta,m,eps_theta,decay_rate,burnin,maxepoch,param_seed)
 * GPT_SGLD.jl:809-847 -> theta_store (n, (maxepoch+burnin)*numbatches) */
int gpt_gpnt_sgld(const double* phi, const double* y, int64_t n, int64_t N, double signal_var,
                  double sigma_theta, int64_t m, double eps_theta, double decay_rate,
                  int64_t burnin, int64_t maxepoch, uint64_t seed, double* theta_store);

/* Sibling GPNT_SGLD chains of one launch on a shared phi / y (step-size, noise and seed sweeps,
 * PowerPlantNoTensorExperiment.jl / kin40kNoTensorExperiment.jl): chain k runs GPNT_SGLD with
 * signal_var[k], sigma_theta[k], eps_theta[k] and seeds[k]; theta0, step noise and epoch orders are
 * gpt_gpnt_sgld's for that seed.  One workgroup per chain keeps theta in LDS for an epoch's steps
 * and reads each feature row of a batch from memory once per step where at least four rows fit
 * beside theta (n up to about 4000 at m = 50; past that the rows are read twice, which measures
 * faster than groups of fewer rows).  store_every >= 1 keeps the 1-based
 * steps divisible by it (1: every step, as the reference; numbatches: the epoch ends; burn-in steps
 * count); theta_store (n, kept, nchains), kept = total steps / store_every.  status[k] =
 * GPT_ERR_NAN_THETA and a zero-filled store for a chain that met a NaN (GPT_SGLD.jl:840-843); the
 * other chains are untouched and the call returns GPT_OK.  theta and the batch's bookkeeping must
 * fit the 160 KiB of LDS (n = 16 000 at m = 50 does); otherwise GPT_ERR_BAD_DIMS.
 * GPTSGLD_GPNT_ROWS=<g> (read on every call) stages min(g, what fits) feature rows per group,
 * 0 = none; the results do not depend on it. */
int gpt_gpnt_sgld_chains(const double* phi, const double* y, int64_t n, int64_t N, int64_t m,
                         const double* signal_var, const double* sigma_theta,
                         const double* eps_theta, double decay_rate, int64_t burnin,
                         int64_t maxepoch, const uint64_t* seeds, int32_t nchains,
                         int64_t store_every, double* theta_store, int32_t* status);
/* The same with phi = featureNotensor(X, length_scale, sigma_rbf, Z, b) formed on the device (the
 * doubles gpt_feature_notensor makes; no n*N host array).  X (N, D) column-major, ls_len 1 or D,
 * Z (n, D), b (n). */
int gpt_gpnt_sgld_chains_x(const double* X, const double* y, int64_t N, int64_t D,
                           const double* length_scale, int64_t ls_len, double sigma_rbf,
                           const double* Z, const double* b, int64_t n, int64_t m,
                           const double* signal_var, const double* sigma_theta,
                           const double* eps_theta, double decay_rate, int64_t burnin,
                           int64_t maxepoch, const uint64_t* seeds, int32_t nchains,
                           int64_t store_every, double* theta_store, int32_t* status);
/* Evaluation of T stored samples theta (n, T) on phitest (n, Ntest) against ytest
 * (PowerPlantNoTensorExperiment.jl:51-63): scores[i, t] = sum_j phitest[j, i]*theta[j, t],
 * sample_rmse_out[t] = scale*||ytest - scores[:, t]||/sqrt(Ntest), mean_out (Ntest) the mean of the
 * scores of the samples avg_first <= t < avg_last (0-based, half open) and *rmse_out the same
 * figure on it; scores_out (Ntest, T) optional.  A null required pointer or a window that is empty
 * or outside [0, T] is GPT_ERR_BAD_DIMS before any kernel runs. */
int gpt_gpnt_pred(const double* theta, const double* phitest, const double* ytest, int64_t n,
                  int64_t Ntest, int64_t T, int64_t avg_first, int64_t avg_last, double scale,
                  double* sample_rmse_out, double* mean_out, double* rmse_out, double* scores_out);
/* The same with phitest = featureNotensor(Xtest, length_scale, sigma_rbf, Z, b) formed on the
 * device. */
int gpt_gpnt_pred_x(const double* theta, const double* Xtest, const double* ytest, int64_t Ntest,
                    int64_t D, const double* length_scale, int64_t ls_len, double sigma_rbf,
                    const double* Z, const double* b, int64_t n, int64_t T, int64_t avg_first,
                    int64_t avg_last, double scale, double* sample_rmse_out, double* mean_out,
                    double* rmse_out, double* scores_out);
/* The route of the last gpt_gpnt_sgld_chains* call on this thread (measurement, for the route
 * assertions of tests/test_gpu_gpnt.py); the first min(len, 3) of: [0] feature rows staged per
 * group (0 = not staged), [1] groups per full batch, [2] dynamic LDS bytes of the sampler's
 * launches.  Entries past 3 are set to 0. */
int gpt_gpnt_last_route(int32_t* out, int32_t len);
/* Device-event times in ms of the last calls on this thread (measurement, scripts/time_gpnt.py):
 * [0] the sampler's launches of gpt_gpnt_sgld_chains*, [1] the scores and reduction kernels of
 * gpt_gpnt_pred*.  Entries past 2 are set to 0. */
int gpt_gpnt_last_timing(double* ms, int32_t len);

/* ---- posterior predictive of the sampled regression models ---------------------------- */
/* The predictive of stored predictions F (Ntest, T) column-major (column s at F + s*Ntest, as
 * gpt_pred_dev and the scores of gpt_gpnt_pred write them) against y (Ntest), over the S = last -
 * first columns first <= s < last (0-based, half open), with Gaussian noise variance noise_var
 * (the model's signal_var).  Per row, in sample order:
 *   fmu   = (sum_s f_s)/S            the bits of gpt_pred_mean / gpt_gpnt_pred's mean on the columns
 *   fs2   = (sum_s (f_s - fmu)^2)/S  two passes, divisor S, the deviations taken about the window's
 *                                    first column; >= 0, and exactly 0 where the columns agree
 *   ymu = fmu, ys2 = fs2 + noise_var  (the equal-weight mixture's mean and variance; not stored)
 *   lp    = -(y - ymu)^2/(2 ys2) - log(2 pi ys2)/2                 GPkit's moment-matched lp
 *   lpmix = log((1/S) sum_s N(y | f_s, noise_var))                 max-shifted logsumexp
 * sums[0] = sum_i lp, sums[1] = sum_i lpmix, *covered = the number of rows with
 * |y - ymu| <= 1.959963984540054 sqrt(ys2) (an integer value): fixed 256-row tiles added in tile
 * order, no atomics, so a repeated call returns the same bits.  A row's outputs depend on its own
 * S values, y and noise_var alone.  The per-row outputs may be NULL.  A null required pointer,
 * Ntest < 1, T outside 1..2^22, an empty window or one outside [0, T], or a noise_var that is not
 * finite and > 0 is GPT_ERR_BAD_DIMS before any device work.
 * The _dev form takes device pointers for F, y and the per-row outputs, writes sums and covered
 * to the host and synchronises hip_stream.  The host form also returns, where asked (both may be
 * NULL), sample_rmse_out[t] = ||y - F[:, t]||/sqrt(Ntest) of all T columns and *rmse_out, the same
 * figure of fmu, from the kernel of gpt_pred_mean. */
int gpt_predictive_dev(const double* F_dev, const double* y_dev, int64_t Ntest, int64_t T,
                       int64_t first, int64_t last, double noise_var, double* fmu_dev,
                       double* fs2_dev, double* lp_dev, double* lpmix_dev, double* sums_host,
                       double* covered_host, void* hip_stream);
int gpt_predictive(const double* F, const double* y, int64_t Ntest, int64_t T, int64_t first,
                   int64_t last, double noise_var, double* fmu_out, double* fs2_out, double* lp_out,
                   double* lpmix_out, double* sums_out, double* covered_out, double* rmse_out,
                   double* sample_rmse_out);
/* gpt_pred_mean's prediction of the S stored tensor samples (the same kernels and routes), then
 * gpt_predictive_dev on the window first <= s < last of them without a copy to the host.
 * sample_rmse_out (S) = scale*||ytest - pred(sample s)||/sqrt(Ntest) and *rmse_out the same figure
 * of fmu are required. */
int gpt_pred_predictive(const double* w_store, const double* U_store, const int32_t* I,
                        const double* phitest, const double* ytest, int64_t n, int64_t D,
                        int64_t Ntest, int64_t r, int64_t Q, int64_t S, double scale, int64_t first,
                        int64_t last, double noise_var, double* fmu_out, double* fs2_out,
                        double* lp_out, double* lpmix_out, double* sums_out, double* covered_out,
                        double* rmse_out, double* sample_rmse_out);
/* The same beside gpt_pred_mean_x: the test features are formed on the device from Xtest
 * (GPTSGLD_PRED=direct as there). */
int gpt_pred_predictive_x(const double* w_store, const double* U_store, const int32_t* I,
                          const double* Xtest, const double* ytest, int64_t Ntest, int64_t D,
                          const double* length_scale, int64_t ls_len, double sigma_rbf,
                          double phi_scale, const double* Z, const double* b, int64_t n, int64_t r,
                          int64_t Q, int64_t S, double scale, int64_t first, int64_t last,
                          double noise_var, double* fmu_out, double* fs2_out, double* lp_out,
                          double* lpmix_out, double* sums_out, double* covered_out,
                          double* rmse_out, double* sample_rmse_out);
/* The same for T stored full-theta samples theta (n, T), beside gpt_gpnt_pred / gpt_gpnt_pred_x:
 * the scores stay on the device; sample_rmse_out (T) and *rmse_out as there. */
int gpt_gpnt_predictive(const double* theta, const double* phitest, const double* ytest, int64_t n,
                        int64_t Ntest, int64_t T, int64_t first, int64_t last, double scale,
                        double noise_var, double* fmu_out, double* fs2_out, double* lp_out,
                        double* lpmix_out, double* sums_out, double* covered_out, double* rmse_out,
                        double* sample_rmse_out);
int gpt_gpnt_predictive_x(const double* theta, const double* Xtest, const double* ytest,
                          int64_t Ntest, int64_t D, const double* length_scale, int64_t ls_len,
                          double sigma_rbf, const double* Z, const double* b, int64_t n, int64_t T,
                          int64_t first, int64_t last, double scale, double noise_var,
                          double* fmu_out, double* fs2_out, double* lp_out, double* lpmix_out,
                          double* sums_out, double* covered_out, double* rmse_out,
                          double* sample_rmse_out);
/* Device-event time in ms of the evaluator's two kernels alone in the last gpt_*predictive* call
 * on this thread (measurement, scripts/time_predictive.py). */
int gpt_predictive_last_timing(double* ms);

/* ---- chain diagnostics of a store: split R-hat, ESS, autocorrelation ------------------- */
/* Diagnostics of store x (P, T, M) column-major: parameter (or test row) p, kept sample s, chain m
 * at store + p + P*(s + T*m).  The window is first <= s < last (0-based, half open), S = last -
 * first >= 4, the lags k = 0..K with K = min(max_lag, S - 1).  Per parameter and chain, in sample
 * order:
 *   chain_mean_m = (sum_s x)/S;  c_s = x_s - chain_mean_m (two passes, the deviations taken about
 *   the chain's first sample, so equal samples give c = 0 exactly);
 *   acov_m(k) = (sum_{s=0}^{S-1-k} c_s c_{s+k})/S (divisor S at every lag);
 *   chain_var_m = acov_m(0)*S/(S - 1);  chain_acf_m(k) = acov_m(k)/acov_m(0).
 * Per parameter, the chains in the order m = 0..M-1:
 *   W = mean_m chain_var_m;  B/S = the variance of the chain means (divisor M - 1; 0 at M = 1);
 *   var+ = W*(S - 1)/S + B/S;  mean = mean_m chain_mean_m;  sd = sqrt(var+);
 *   acf[k] = 1 - (W - mean_m acov_m(k))/var+            (the combined rho_k of BDA3 11.5 / Stan)
 *   Geyer's initial monotone sequence: P_j = acf[2j] + acf[2j+1] for 2j + 1 <= K, stopped at the
 *   first P_j <= 0, else P_j = min(P_j, P_{j-1});  tau = max(-1 + 2 sum_j P_j, 1/log10(M*S));
 *   ess = M*S/tau;  mcse = sd/sqrt(ess);  truncated = 1 when the lags ran out before a stop (ess
 *   is then an upper bound: max_lag too small, or chains that disagree);
 *   split R-hat: H = floor(S/2), the first and the last H samples of every chain (the middle one
 *   dropped at odd S) as 2M sequences, W_h the mean of their variances (divisor H - 1), B_h/H the
 *   variance of their means (divisor 2M - 1), rhat = sqrt(((H - 1)/H*W_h + B_h/H)/W_h).
 * A parameter with var+ == 0 is constant: its rhat, ess, mcse, tau and acf are NaN, truncated 0.
 * No atomics; every sum runs in an order fixed by S and K; a parameter's results depend on its
 * own values alone, a chain's chain_mean, chain_var and chain_acf on that chain's alone, and
 * acf[k] has the same bits for every max_lag >= k.
 * Outputs: mean, sd, rhat, ess, mcse, tau, truncated (P each); optional (NULL to skip) chain_mean
 * and chain_var (P, M), acf (P, K+1) and chain_acf (P, K+1, M).  GPT_ERR_BAD_DIMS with a message
 * before any device work for a null required pointer, P < 1, T outside 4..2^22, M outside 1..1024,
 * max_lag outside 1..4096, a window outside 0 <= first < last <= T or shorter than 4, and, for the
 * host entry, a store of more than 2^31 doubles (16 GiB, one upload).
 * The _dev form takes device pointers throughout and chain m at store + chain_stride*m
 * (chain_stride >= P*T elements: separately allocated (P, T) predictions at a constant stride need
 * no copy); it synchronises hip_stream. */
int gpt_chain_diag(const double* store, int64_t P, int64_t T, int64_t M, int64_t first,
                   int64_t last, int64_t max_lag, double* mean, double* sd, double* rhat,
                   double* ess, double* mcse, double* tau, int32_t* truncated, double* chain_mean,
                   double* chain_var, double* acf, double* chain_acf);
int gpt_chain_diag_dev(const double* store_dev, int64_t P, int64_t T, int64_t M,
                       int64_t chain_stride, int64_t first, int64_t last, int64_t max_lag,
                       double* mean_dev, double* sd_dev, double* rhat_dev, double* ess_dev,
                       double* mcse_dev, double* tau_dev, int32_t* truncated_dev,
                       double* chain_mean_dev, double* chain_var_dev, double* acf_dev,
                       double* chain_acf_dev, void* hip_stream);
/* Device-event time in ms of the evaluator's kernels alone in the last gpt_chain_diag* call on
 * this thread (measurement, scripts/time_diag.py). */
int gpt_diag_last_timing(double* ms);
/* out[0..2] = the samples per time chunk, the lags per wave and the lags per workgroup of the
 * autocovariance kernel (the edges the tests place their shapes at); entries past 2 are 0. */
int gpt_diag_tiling(int32_t* out, int32_t len);

/* ---- classification: the full-theta softmax sampler and the evaluation of scores ------ */
/* GPNT_SGLDclass(phi,y,sigma_theta,m,eps_theta,decay_rate,burnin,maxepoch,param_seed)
 * GPT_SGLD.jl:851-901.  phi (n, N); y (N) integer labels in 1..C, C = max(y) - min(y) + 1 <= 32
 * (anything else is GPT_ERR_BAD_DIMS); theta_store (n, C, (burnin+maxepoch)*numbatches).
 * RNG: theta[:, c] = sigma_theta*normals(n, seed, 0, THETA_INIT, c); the noise of 1-based step t
 * and class c is normals(n, seed, t-1, THETA_NOISE, c); epoch orders as GPNT_SGLD.  As the
 * reference, the prior term of the gradient is +theta (sigma_theta scales the initial draw only).
 * A NaN in theta returns GPT_ERR_NAN_THETA with a zero-filled store (:894-897). */
int gpt_gpnt_sgld_class(const double* phi, const double* y, int64_t n, int64_t N,
                        double sigma_theta, int64_t m, double eps_theta, double decay_rate,
                        int64_t burnin, int64_t maxepoch, uint64_t seed, double* theta_store);
/* Sibling chains of one launch on a shared phi / y (step-size and seed sweeps,
 * ImageNoTensorExperiment.jl:36-38): chain k runs GPNT_SGLDclass with eps_theta[k] and seeds[k],
 * labels in 1..ncls.  store_every >= 1 keeps the 1-based steps divisible by it (1: every step, as
 * the reference; numbatches: the epoch ends); theta_store (n, ncls, kept, nchains), kept =
 * total steps / store_every.  status[k] = GPT_ERR_NAN_THETA and a zero-filled store for a chain
 * that met a NaN; the other chains are untouched and the call returns GPT_OK. */
int gpt_gpnt_sgld_class_chains(const double* phi, const double* y, int64_t n, int64_t N,
                               int64_t ncls, double sigma_theta, int64_t m, const double* eps_theta,
                               double decay_rate, int64_t burnin, int64_t maxepoch,
                               const uint64_t* seeds, int32_t nchains, int64_t store_every,
                               double* theta_store, int32_t* status);
/* Evaluation of class scores (ImageExperiment.jl:50-72, ImageNoTensorExperiment.jl:50-75).
 * scores (Ntest, C, T) column-major, ytest (Ntest) labels in 1..C.  Per sample t:
 *   prop_missed_out[t] = 1 - #(indmax(scores[i,:,t]) == ytest[i])/Ntest (ties: the first index),
 *   mean_nlp_out[t] = mean_i (logsumexp(scores[i,:,t]) - scores[i,ytest[i],t]),
 * and the same two figures, avg_out[0] and avg_out[1], on mean_scores (Ntest, C), the mean of
 * the samples avg_first <= t < avg_last (0-based, half open).  Optional outputs (may be NULL):
 * mean_scores_out (Ntest, C), prediction_out (Ntest, 1-based) and nlp_out (Ntest) of the
 * averaged scores.  A null required pointer, an empty window or one outside [0, T], or a label
 * outside 1..C is GPT_ERR_BAD_DIMS before any kernel runs. */
int gpt_class_eval(const double* scores, const int32_t* ytest, int64_t Ntest, int64_t C, int64_t T,
                   int64_t avg_first, int64_t avg_last, double* prop_missed_out,
                   double* mean_nlp_out, double* avg_out, double* mean_scores_out,
                   int32_t* prediction_out, double* nlp_out);
/* The same on device pointers (the labels are read back once to be checked); synchronises
 * hip_stream. */
int gpt_class_eval_dev(const double* scores_dev, const int32_t* ytest_dev, int64_t Ntest, int64_t C,
                       int64_t T, int64_t avg_first, int64_t avg_last, double* prop_missed_dev,
                       double* mean_nlp_dev, double* avg_dev, double* mean_scores_dev,
                       int32_t* prediction_dev, double* nlp_dev, void* hip_stream);
/* Full-theta evaluation: scores[i, c, t] = sum_j phitest[j, i]*theta[j, c, t] for theta (n, C, T)
 * and phitest (n, Ntest) in one launch, then gpt_class_eval on them; scores_out (Ntest, C, T)
 * optional. */
int gpt_gpnt_pred_class(const double* theta, const double* phitest, const int32_t* ytest, int64_t n,
                        int64_t Ntest, int64_t C, int64_t T, int64_t avg_first, int64_t avg_last,
                        double* prop_missed_out, double* mean_nlp_out, double* avg_out,
                        double* mean_scores_out, int32_t* prediction_out, double* nlp_out,
                        double* scores_out);
/* Tensor evaluation of GPTclassification's stores: w (Q, C, T), U (n, r, D, C, T), I (Q, D)
 * 1-based, phitest (n, D, Ntest) uploaded once; the scores are gpt_pred_dev's on the S = C*T
 * stacked samples (same routes, passes and environment switches, and the same shape limits),
 * then gpt_class_eval on them; scores_out (Ntest, C, T) optional. */
int gpt_pred_class(const double* w, const double* U, const int32_t* I, const double* phitest,
                   const int32_t* ytest, int64_t n, int64_t D, int64_t Ntest, int64_t r, int64_t Q,
                   int64_t C, int64_t T, int64_t avg_first, int64_t avg_last,
                   double* prop_missed_out, double* mean_nlp_out, double* avg_out,
                   double* mean_scores_out, int32_t* prediction_out, double* nlp_out,
                   double* scores_out);

/* Device-event times in ms of the last classification calls on this thread (measurement,
 * scripts/time_class.py): ms_out[0] the sampler's launches, [1] the scores (nt_scores_kernel, or
 * the stacked-sample prediction of gpt_pred_class), [2] the evaluation kernels. */
int gpt_class_last_timing(double* ms_out);

/* ---- full-theta model: hyper-parameter learning -------------------------------------- */
/* GPNT_nlogmarginal / GPNT_gradnlogmarginal (GPT_SGLD.jl:921-962) with featureNotensor and
 * gradfeatureNotensor (:109-120, :142-177) as the feature closures: the negative log marginal
 * likelihood of the no-tensor RFF GP and its gradient with respect to
 *   hyper = [length_scale (D entries, or 1: the scalar form); sigma_RBF; signal_var],
 * Lh = D + 2 or 3.  X (N, D), y (N), Z (n, D), b (n); n <= 1024 (the single-workgroup Cholesky),
 * D <= 16.  A hyper-parameter that is not positive and finite, or a dimension out of range, is
 * GPT_ERR_BAD_DIMS before any device call.  When phi*phi' + signal_var*I fails its Cholesky
 * factorisation (a NaN in X, for one) the call returns GPT_ERR_NOT_SPD and fills nlml, grad
 * and theta_mean with NaN.
 *
 * The evaluator keeps X, y, Z, b and its scratch on the device, so an optimiser's evaluations
 * upload only the hyper-parameters.  grad (Lh) may be NULL when want_grad = 0; theta_mean (n,
 * optional) receives l = A^-1 phi y, the posterior mean of the full-theta weights at hyper. */
typedef struct gpt_nlml gpt_nlml;
int gpt_nlml_create(const double* X, int64_t N, int64_t D, const double* y, const double* Z,
                    const double* b, int64_t n, gpt_nlml** out);
int gpt_nlml_eval(gpt_nlml* h, const double* hyper, int64_t Lh, int32_t want_grad, double* nlml,
                  double* grad, double* theta_mean);
/* Test entry: phi (n, N) of the last evaluation and S = c*sin(f) of the last one with
 * want_grad (either may be NULL). */
int gpt_nlml_features(gpt_nlml* h, double* phi_out, double* sin_out);
/* Diagnostics (scripts/time_nlml.py): gpt_nlml_eval with device-event times in ms of its 11
 * phases: features, SYRK, GEMV, Cholesky, the two triangular solves, L^-T, P = A^-1, e, the
 * gradient GEMM, its finish, the scalar sums (the gradient's five are 0 when want_grad = 0). */
int gpt_nlml_eval_timed(gpt_nlml* h, const double* hyper, int64_t Lh, int32_t want_grad,
                        double* nlml, double* grad, double* phase_ms);
int gpt_nlml_destroy(gpt_nlml* h);
/* One-shot host-pointer form (create, one evaluation, destroy). */
int gpt_gpnt_nlogmarginal(const double* X, int64_t N, int64_t D, const double* y, const double* Z,
                          const double* b, int64_t n, const double* hyper, int64_t Lh,
                          int64_t want_grad, double* nlml_out, double* grad_out);

/* ---- full-theta model: closed-form predictive and kernel approximation error ---------- */
/* The posterior of GPNT_nlogmarginal's model (y = phi(x)'theta + eps, theta ~ N(0, I), eps ~
 * N(0, signal_var)) is theta | y ~ N(l, signal_var*A^-1) with A = phi*phi' + signal_var*I = L*L'
 * and l = A^-1 phi y.  For Xtest (Ntest, D) column-major and phis = featureNotensor(Xtest):
 *   fmu = phis'l,  fs2 = signal_var * colsum((L^-1 phis)^2)   (ymu = fmu, ys2 = fs2 + signal_var)
 * and, with ytest and lp, lp = -(ytest - fmu)^2/(2 ys2) - log(2 pi ys2)/2: GPkit's prediction
 * with LikGauss, the outputs of gpt_egp_predict.  fs2 is a sum of squares: positive, no clamp.
 * The test rows go through the device in chunks of `chunk` columns (0: the library's choice; at
 * most 4096); a row's results depend neither on the chunking, nor on Ntest, nor on the row's
 * position.  The factor of the last successful evaluation is reused when hyper equals its hyper
 * bit for bit, otherwise the call evaluates first; the results are the same bits either way.
 * Ntest < 1 or a NULL array is GPT_ERR_BAD_DIMS; a failed Cholesky returns GPT_ERR_NOT_SPD with
 * NaN-filled outputs and leaves the handle usable. */
int gpt_nlml_predict(gpt_nlml* h, const double* hyper, int64_t Lh, const double* Xtest,
                     int64_t Ntest, const double* ytest, int64_t chunk, double* fmu, double* fs2,
                     double* lp);
/* One-shot host-pointer form (create, predict, destroy). */
int gpt_gpnt_predict(const double* X, int64_t N, int64_t D, const double* y, const double* Z,
                     const double* b, int64_t n, const double* hyper, int64_t Lh,
                     const double* Xtest, int64_t Ntest, const double* ytest, double* fmu,
                     double* fs2, double* lp);
/* The live code of PowerPlantDataExperiment.jl:47-97: with K_ij = sigma_RBF^2 exp(-1/2 sum_k
 * ((x_ik - x_jk)/l_k)^2) (the exact GP's covariance, no noise term) and K_rff = phi'phi,
 * phi = featureNotensor(X), over all N^2 entries
 *   out3 = { |K - K_rff|_F (the reference's FrobError), |K|_F, max |K - K_rff| }.
 * Neither matrix is stored (phi is: n*N doubles).  X (N, D), Z (n, D), b (n); hyper as above
 * (signal_var is validated and unused).  No Cholesky, so n may exceed 1024: n <= 8192,
 * N <= 65536, D <= 16 and 8*n*N <= 2 GiB; beyond them GPT_ERR_BAD_DIMS.  Equal inputs give
 * equal bits. */
int gpt_rff_kernel_error(const double* X, int64_t N, int64_t D, const double* Z, const double* b,
                         int64_t n, const double* hyper, int64_t Lh, double* out3);
/* Diagnostics (scripts/time_rffgp.py): device-event times in ms of this thread's last calls:
 * ms[0] gpt_rff_kernel_error's features, ms[1] its tile pass and finish, ms[2] the chunks of
 * gpt_nlml_predict (the uploads of their rows included). */
int gpt_rff_last_timing(double* ms, int32_t len);

/* ---- hyper-parameter learning of the softmax classifier: the joint likelihood ---------- */
/* neglogjointlkhd / gradneglogjointlkhd (ImageExperiment.jl:135-204), the objective of
 * GPNT_hyperparameters_ng (GPT_SGLD.jl:1005-1063): with phi = featureNotensor(X) at
 *   hyper = [length_scale (D entries, or 1: the scalar form); sigma_RBF],  Lh = D + 1 or 2,
 * and s = theta'phi (C, N),
 *   value = sum_i (logsumexp(s[:, i]) - s[y_i, i]) + |theta|^2/2,
 * and its gradient with respect to theta (n, C) and hyper.  X (N, D), Z (n, D), theta (n, C)
 * column-major; y (N) doubles holding integers in 1..C (a class may be absent); n <= 1024,
 * D <= 16, C <= 32.  A dimension out of range, a label that is no integer in 1..C, a NULL array
 * or a hyper-parameter that is not positive and finite is GPT_ERR_BAD_DIMS before any kernel.
 *
 * The evaluator keeps X, y, Z, b, theta and its scratch on the device; nothing of size n*N is
 * stored.  Equal inputs give equal bits, and want_grad = 0 returns the value bits of a gradient
 * evaluation.  gpt_cjoint_eval: theta (n, C) is uploaded and becomes the resident one, NULL
 * means the resident theta (zero after create); grad_theta (n*C) and grad_hyper (Lh) may be
 * NULL. */
typedef struct gpt_cjoint gpt_cjoint;
int gpt_cjoint_create(const double* X, int64_t N, int64_t D, const double* y, int64_t C,
                      const double* Z, const double* b, int64_t n, gpt_cjoint** out);
int gpt_cjoint_eval(gpt_cjoint* h, const double* hyper, int64_t Lh, const double* theta,
                    int32_t want_grad, double* value, double* grad_theta, double* grad_hyper);
int gpt_cjoint_set_theta(gpt_cjoint* h, const double* theta);
int gpt_cjoint_get_theta(gpt_cjoint* h, double* theta_out);
/* nsteps Langevin steps on the resident theta at hyper with no host round trip
 * (GPT_SGLD.jl:1031-1033): theta <- theta - (eps/2*grad_theta + sqrt(eps)*xi), where xi of 0-based
 * step t, feature j and class c is element j of the normal stream (seed, t, THETA_NOISE, c), the
 * contract of gpt_gpnt_sgld_class.  The handle keeps the counter of the next step (0 after
 * create, gpt_cjoint_steps reads it): t0 >= 0 sets it first, t0 < 0 continues.  When theta turns
 * non-finite the remaining steps are not taken and the call returns GPT_ERR_NAN_THETA. */
int gpt_cjoint_langevin(gpt_cjoint* h, const double* hyper, int64_t Lh, double eps, int64_t nsteps,
                        uint64_t seed, int64_t t0);
int gpt_cjoint_steps(gpt_cjoint* h, int64_t* step_out);
/* Hamiltonian Monte Carlo on the resident theta at hyper, burnin + nsamples transitions with no
 * host round trip.  U(theta) is the value above (the prior |theta|^2/2 included), H = U + |p|^2/2
 * and eps is the squared step, s = sqrt(eps); L = 1 is the MALA loop of
 * BloodTransfusionExperiment.jl:255-278.  0-based transition t (the counter of
 * gpt_cjoint_langevin: t0 >= 0 sets it first, t0 < 0 continues):
 *   p[j, c] = element j of the normal stream (seed, t, HMC_MOM = 26, c);
 *   p -= s/2 grad U(theta), q = theta + s p; L - 1 times p -= s grad U(q), q += s p;
 *   p -= s/2 grad U(q);  u = the uniform of (seed, t, HMC_ACCEPT = 27, 0);
 *   theta <- q iff u < exp(H0 - H1); otherwise theta keeps its bits.
 * A non-finite H1 rejects and is counted in *ndivergent_out; it is no error.  theta_store
 * (n, C, nsamples/thin) takes theta after every thin-th transition past burn-in; accept_out, dH_out
 * (H0 - H1) and value_out (U of the kept state) take one entry per transition, burn-in included.
 * Every output may be NULL.  U and grad U of the kept state are cached across transitions and
 * calls, so a transition costs L evaluations; set_theta, eval with a theta, langevin or other
 * hyper bits drop the cache, and the result is bit for bit that of recomputing.
 * GPT_ERR_BAD_DIMS before any kernel: eps not positive and finite, L outside 1..1024, thin < 1,
 * burnin or nsamples outside 0..2^24, a counter that would pass 2^32, bad hyper.
 * GPT_ERR_NAN_THETA before any transition: the starting theta or U(theta) is not finite. */
int gpt_chmc_run(gpt_cjoint* h, const double* hyper, int64_t Lh, double eps, int64_t L,
                   int64_t burnin, int64_t nsamples, int64_t thin, uint64_t seed, int64_t t0,
                   double* theta_store, int32_t* accept_out, double* dH_out, double* value_out,
                   int64_t* ndivergent_out);
/* The integrator alone: L leapfrog steps from the resident theta (unchanged) on the momentum
 * p_inout (n, C), which takes the final momentum; q_out (n, C) the final position, H_out = [H0, H1].
 * q_out and H_out may be NULL. */
int gpt_chmc_leapfrog(gpt_cjoint* h, const double* hyper, int64_t Lh, double eps, int64_t L,
                        double* p_inout, double* q_out, double* H_out);
/* scores (Ntest, C) = featureNotensor(Xtest)'theta at hyper for the resident theta: the block
 * gpt_class_eval reads as one sample.  The _dev form takes device pointers and a hipStream_t and
 * does not synchronise. */
int gpt_cjoint_scores(gpt_cjoint* h, const double* hyper, int64_t Lh, const double* Xtest,
                      int64_t Ntest, double* scores_out);
int gpt_cjoint_scores_dev(gpt_cjoint* h, const double* hyper, int64_t Lh, const double* Xtest_dev,
                          int64_t Ntest, double* scores_dev, void* hip_stream);
/* The scores of the test rows, kept on the device, through gpt_class_eval_dev as one sample
 * (ImageExperiment.jl:258-268): outputs as gpt_class_eval with T = 1; scores_out (Ntest, C)
 * optional. */
int gpt_cjoint_class_eval(gpt_cjoint* h, const double* hyper, int64_t Lh, const double* Xtest,
                          const int32_t* ytest, int64_t Ntest, double* prop_missed_out,
                          double* mean_nlp_out, double* avg_out, double* mean_scores_out,
                          int32_t* prediction_out, double* nlp_out, double* scores_out);
/* Diagnostics (scripts/time_cjoint.py): device-event time in ms per evaluation over reps
 * back-to-back evaluations in mode 0 (value), 1 (value and grad_theta partials), 2 (the full
 * gradient) or 4 (the features phi and S of every tile alone). */
int gpt_cjoint_time(gpt_cjoint* h, const double* hyper, int64_t Lh, int32_t mode, int32_t reps,
                    double* ms_out);
int gpt_cjoint_destroy(gpt_cjoint* h);
/* One-shot host-pointer forms (create, one call, destroy).  grad_out (n*C + Lh) =
 * [vec(grad_theta); grad_length_scale; grad_sigma_RBF], the reference's layout.
 * gpt_gpnt_joint_langevin updates theta in place from step t0 >= 0; gpt_gpnt_joint_scores needs
 * no training data. */
int gpt_gpnt_neglogjoint(const double* X, int64_t N, int64_t D, const double* y, int64_t C,
                         const double* Z, const double* b, int64_t n, const double* theta,
                         const double* hyper, int64_t Lh, int64_t want_grad, double* value_out,
                         double* grad_out);
int gpt_gpnt_joint_langevin(const double* X, int64_t N, int64_t D, const double* y, int64_t C,
                            const double* Z, const double* b, int64_t n, double* theta,
                            const double* hyper, int64_t Lh, double eps, int64_t nsteps,
                            uint64_t seed, int64_t t0);
/* gpt_chmc_run from host arrays: theta (n, C) is the start and takes the final state, t0 >= 0;
 * the divergent count (at most 2^25 transitions) is a 32-bit integer here. */
int gpt_gpnt_joint_hmc(const double* X, int64_t N, int64_t D, const double* y, int64_t C,
                       const double* Z, const double* b, int64_t n, double* theta,
                       const double* hyper, int64_t Lh, double eps, int64_t L, int64_t burnin,
                       int64_t nsamples, int64_t thin, uint64_t seed, int64_t t0,
                       double* theta_store, int32_t* accept_out, double* dH_out, double* value_out,
                       int32_t* ndivergent_out);
int gpt_gpnt_joint_scores(const double* Xtest, int64_t Ntest, int64_t D, int64_t C, const double* Z,
                          const double* b, int64_t n, const double* theta, const double* hyper,
                          int64_t Lh, double* scores_out);

/* ---- exact GP regression (the reference's quality ceiling) ------------------------------ */
/* GP_nlogmarginal (GPT_SGLD.jl:905-915) and GPkit's InfExact / prediction with CovSEiso or
 * CovSEard, LikGauss and a zero mean: K_ij = sigma_RBF^2 exp(-1/2 sum_k ((x_ik - x_jk)/l_k)^2),
 * A = K + signal_var*I = L*L', alpha = A^-1 y,
 *   nlml = sum log L_ii + y'alpha/2 + (N/2) log 2 pi,
 * and its gradient with respect to
 *   hyper = [length_scale (D entries, or 1: the iso form); sigma_RBF; signal_var],
 * Lh = D + 2 or 3 (GPkit's dnlZ is this gradient times l_k, sigma_RBF and 2*signal_var).
 * X (N, D) column-major, y (N); N <= 16384, D <= 16.  A hyper-parameter that is not positive and
 * finite, a dimension out of range or a NULL array is GPT_ERR_BAD_DIMS before any device call or
 * allocation.  When the blocked Cholesky meets a pivot that is not positive the call returns
 * GPT_ERR_NOT_SPD with NaN-filled outputs and the handle stays usable.
 *
 * The evaluator keeps X, y, the factor and its scratch on the device (N*N doubles, and two more
 * N*N buffers from the first gradient on).  grad (Lh) may be NULL when want_grad = 0; alpha (N,
 * optional) receives A^-1 y. */
typedef struct gpt_egp gpt_egp;
int gpt_egp_create(const double* X, int64_t N, int64_t D, const double* y, gpt_egp** out);
int gpt_egp_eval(gpt_egp* h, const double* hyper, int64_t Lh, int32_t want_grad, double* nlml,
                 double* grad, double* alpha);
/* Diagnostics (scripts/time_exactgp.py): gpt_egp_eval with device-event times in ms of its 6
 * phases: kernel matrix, Cholesky, the vector solves, L^-1, P = A^-1, the gradient pass (the last
 * three are 0 when want_grad = 0). */
int gpt_egp_eval_timed(gpt_egp* h, const double* hyper, int64_t Lh, int32_t want_grad,
                       double* nlml, double* grad, double* phase_ms);
/* GPkit prediction at hyper for Xtest (Ntest, D) column-major: fmu = Ks'alpha, fs2 =
 * max(sigma_RBF^2 - colsum((L^-1 Ks)^2), 0) (ymu = fmu, ys2 = fs2 + signal_var) and, with ytest
 * and lp, lp = -(ytest - fmu)^2/(2 ys2) - log(2 pi ys2)/2.  The test rows go through the device in
 * chunks of `chunk` columns (0: the library's choice; at most 4096); a row's results do not depend
 * on the chunking.  The factor of the last successful evaluation is reused when hyper equals its
 * hyper bit for bit, otherwise the call fits first. */
int gpt_egp_predict(gpt_egp* h, const double* hyper, int64_t Lh, const double* Xtest,
                    int64_t Ntest, const double* ytest, int64_t chunk, double* fmu, double* fs2,
                    double* lp);
int gpt_egp_destroy(gpt_egp* h);
/* One-shot host-pointer forms (create, one call, destroy). */
int gpt_gp_nlogmarginal(const double* X, int64_t N, int64_t D, const double* y,
                        const double* hyper, int64_t Lh, int64_t want_grad, double* nlml_out,
                        double* grad_out);
int gpt_gp_predict(const double* X, int64_t N, int64_t D, const double* y, const double* hyper,
                   int64_t Lh, const double* Xtest, int64_t Ntest, const double* ytest,
                   double* fmu, double* fs2, double* lp);

/* ---- function draws: GP prior and posterior, RFF posterior weights --------------------- */
/* Common to the draw entries below.  S draws come from M x S standard normals Z (column-major; M =
 * N, Ntest or n): Zin (M*S, optional) when given, for common random numbers, else element (i, s) =
 * the Philox normal (seed, e = i, c1 = s, c2 = 25, c3 = kind), kind 0 prior, 1 posterior, 2 theta,
 * so that column s does not depend on S.  Zout (M*S, optional) receives the normals used.  A draw
 * is its mean plus c*T*z for a triangular factor T, summed in an order fixed by M alone: column s
 * of the result depends on column s of Z only, not on S or the other columns, and equal calls give
 * equal bits.  S is in 1..4096, jitter >= 0 and finite; otherwise, and for a NULL required array,
 * GPT_ERR_BAD_DIMS before any device call.  A factorisation that meets a pivot that is not
 * positive returns GPT_ERR_NOT_SPD with every output NaN-filled and a message naming the matrix;
 * the handle stays usable.  Calls on one handle interleave in any order with eval / predict. */
/* GPrand (GaussianProcess.jl:66-80) at the handle's X: F (N, S) = R'z with R = chol(K +
 * jitter*I).  hyper = [length_scale; sigma_RBF; signal_var] as everywhere; signal_var is validated
 * and unused, GPrand adds the jitter alone.  The call invalidates the handle's factor (the next
 * predict refits). */
int gpt_egp_draw_prior(gpt_egp* h, const double* hyper, int64_t Lh, double jitter, int64_t S,
                       uint64_t seed, const double* Zin, double* F, double* Zout);
/* GPpost followed by GPrand (GaussianProcess.jl:82-122): the posterior GP at Xtest (Ntest, D),
 * Ntest in 1..8192, on the factor of the last evaluation at hyper (as gpt_egp_predict; it fits
 * otherwise).  fmu (Ntest, optional) is gpt_egp_predict's, bit for bit; cov (Ntest*Ntest,
 * optional) the joint covariance k(x,x') - k(x)'(K + signal_var*I)^-1 k(x'), full symmetric,
 * neither jitter nor signal_var included; F (Ntest, S, optional) = fmu + L*z with L*L' = cov +
 * d*I, d = jitter (observed = 0: function values) or jitter + signal_var (observed = 1:
 * observations).  With F NULL, S = 0 is allowed and Zin / Zout are ignored. */
int gpt_egp_draw_posterior(gpt_egp* h, const double* hyper, int64_t Lh, const double* Xtest,
                           int64_t Ntest, double jitter, int32_t observed, int64_t S,
                           uint64_t seed, const double* Zin, double* fmu, double* F, double* cov,
                           double* Zout);
/* Exact draws from the posterior of GPNT_nlogmarginal's model (GPT_SGLD.jl:921-933), theta | y ~
 * N(l, signal_var*A^-1): theta (n, S) = l + sqrt(signal_var)*L^-T z, in the layout of a GPNT_SGLD
 * store.  The factor is reused or built as in gpt_nlml_predict. */
int gpt_nlml_draw_theta(gpt_nlml* h, const double* hyper, int64_t Lh, int64_t S, uint64_t seed,
                        const double* Zin, double* theta, double* Zout);
/* One-shot GPrand (GaussianProcess.jl:66-80; MakeSynthData.jl:31-60 draws its regression set with
 * it): create, gpt_egp_draw_prior, destroy.  F (N, S). */
int gpt_gp_rand(const double* X, int64_t N, int64_t D, const double* hyper, int64_t Lh,
                double jitter, int64_t S, uint64_t seed, double* F);
/* One-shot host-pointer forms of the two above (create, one call, destroy), as gpt_gp_predict and
 * gpt_gpnt_predict are of the predictions: the same bits as the handle forms. */
int gpt_gp_post_rand(const double* X, int64_t N, int64_t D, const double* y, const double* hyper,
                     int64_t Lh, const double* Xtest, int64_t Ntest, double jitter,
                     int32_t observed, int64_t S, uint64_t seed, const double* Zin, double* fmu,
                     double* F, double* cov);
int gpt_gpnt_draw_theta(const double* X, int64_t N, int64_t D, const double* y, const double* Z,
                        const double* b, int64_t n, const double* hyper, int64_t Lh, int64_t S,
                        uint64_t seed, const double* Zin, double* theta);
/* Diagnostics (scripts/time_gpdraw.py): device-event times in ms of this thread's last draw call:
 * normals, kernel assembly, solves, covariance, Cholesky, triangular product. */
int gpt_gpdraw_last_timing(double* ms, int32_t len);

/* ---- tensor-GP Gibbs sampler (§8 a25) ----------------------------------------------- */
/* GPT_inf(b,y,sigma,n,r,q,num_iterations,burnin) TGP.jl:37-86 on whitened data.
 * b (n, D, N) column-major feature array (TGP.feature, TGP.jl:6-14), y (N).
 * I (q, D) 1-based core indices; NULL draws them (TGP.jl:50) on the TGP_I Philox stream, and
 * I_out (optional) receives the indices used.  U starts at sqrt(1/r)·randn (TGP.jl:48-49,
 * TGP_U_INIT stream).  W_out (q, T), U_out (n, r, D, T), T = num_iterations - burnin: the W
 * draw of each kept sweep and the U it was drawn against (TGP.jl:60-63).
 * Returns GPT_ERR_NOT_SPD when a precision matrix is not positive definite. */
int gpt_tgp_gibbs(const double* b, const double* y, int64_t n, int64_t D, int64_t N, int64_t r,
                  int64_t q, double sigma, int64_t num_iterations, int64_t burnin, uint64_t seed,
                  const int32_t* I, double* W_out, double* U_out, int32_t* I_out);

/* ---- geodesic Monte Carlo (§8(f) item 4) ------------------------------------------- */
/* GPT_GMC(phi,y,signal_var,I,r,Q,epsw,epsU,burnin,maxepoch,L,param_seed)  GPT_SGLD.jl:684-805:
 * full-batch HMC with L leapfrog steps per epoch (Stiefel geodesic drift for U, geodboth
 * :40-59), sigma_w = 1.  w_store (Q, maxepoch), U_store (n, r, D, maxepoch), accept_prob
 * (burnin+maxepoch).  As the reference, a rejection restores w only (U_old aliases U there).
 * Optional w_init (Q) / U_init (n, r, D).  GPT_ERR_NAN_GEODESIC: zero stores, NaN accept_prob. */
int gpt_gmc(const double* phi, const double* y, int64_t n, int64_t D, int64_t N, int64_t r,
            int64_t Q, const int32_t* I, double signal_var, double epsw, double epsU,
            int64_t burnin, int64_t maxepoch, int64_t L, uint64_t seed, const double* w_init,
            const double* U_init, double* w_store, double* U_store, double* accept_prob);

/* ---- MovieLens-100k tensor CF with side information (§8(f) item 1, config 5) -------- */
/* GPT_fullw_sideinfo(Rating,UserData,MovieData,Ratingtest,signal_var,sigma_u,sigma_w,w_init,m,
 *   epsw,epsU,a,b,c,burnin,maxepoch,param_seed,ytrainMean,ytrainStd;langevin,stiefel,avg)
 * 100k_movielensExperiment.jl:409-551.  Rating (N x >=3, leading dimension ldr, column-major):
 * 1-based user, movie, standardised rating; Ratingtest likewise (ldt).  UserData (n1 x D1),
 * MovieData (n2 x D2) column-major 0/1 side information; w_init (r x r).  Outputs (caller-
 * allocated, column-major): w_store (r,r,maxepoch), U_store (n1+D1,r,maxepoch), V_store
 * (n2+D2,r,maxepoch), testpred_store (Ntest,maxepoch), trainRMSE / testRMSE (maxepoch; epochs
 * after the early stop of :545-547 keep 0 / 10).  GPT_ERR_NAN_GEODESIC: zero parameter stores. */
int gpt_cf_fullw_sideinfo(const double* Rating, int64_t N, int64_t ldr, const double* UserData,
                          int64_t n1, int64_t D1, const double* MovieData, int64_t n2, int64_t D2,
                          const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var,
                          double sigma_u, double sigma_w, const double* w_init, int64_t r, int64_t m,
                          double epsw, double epsU, double a, double b, double c, int64_t burnin,
                          int64_t maxepoch, uint64_t seed, double ytrainMean, double ytrainStd,
                          int32_t langevin, int32_t stiefel, int32_t avg, double* w_store,
                          double* U_store, double* V_store, double* testpred_store,
                          double* trainRMSE, double* testRMSE);

/* GPT_fullw_gibbs(Rating,UserData,MovieData,Ratingtest,signal_var,sigma_u,sigma_w,w_init,burnin,
 *   maxepoch,n_samples,param_seed;avg,rotated_w)  100k_movielensExperiment.jl:1032-1129: Gibbs
 * sweeps of the CF model without side information (U: n1 x r, V: n2 x r rows | the rest, then
 * w | U, V through the N x r^2 Kronecker design).  n1 / n2 are size(UserData,1) / size(MovieData,1);
 * ytrainMean / ytrainStd are arguments (the reference reads script globals).  Outputs as
 * gpt_cf_fullw_sideinfo with U_store (n1,r,maxepoch), V_store (n2,r,maxepoch).
 * GPT_ERR_NOT_SPD on a non positive definite precision (Julia's PosDefException): detected within
 * two epochs of the failed Cholesky, and every output array is zeroed (the reference returns none). */
int gpt_cf_fullw_gibbs(const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
                       const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var,
                       double sigma_u, double sigma_w, const double* w_init, int64_t r,
                       int64_t burnin, int64_t maxepoch, int64_t n_samples, uint64_t seed,
                       double ytrainMean, double ytrainStd, int32_t avg, int32_t rotated_w,
                       double* w_store, double* U_store, double* V_store, double* testpred_store,
                       double* trainRMSE, double* testRMSE);

/* The folds of 100k_movielensExperiment.jl:733-736 (`@parallel for i=1:5` over
 * GPT_fullw_sideinfo(Ratingtrain[:,:,i], ..., Ratingtest[:,:,i], ..., ytrainMean[i],
 * ytrainStd[i])) as F sibling chains of one device launch per epoch: fold f reads Rating[f]
 * (N[f] x >=3, column-major, leading dimension N[f]) and Ratingtest[f] (Ntest[f] x >=3) and
 * writes w_store[f] .. testRMSE[f] exactly as F separate gpt_cf_fullw_sideinfo calls with the
 * same param_seed would (same init, per-epoch permutation and early stop, per fold); every fold
 * has the same N.  status[f] (optional): GPT_OK or GPT_ERR_NAN_GEODESIC for that fold; the return
 * value is GPT_ERR_NAN_GEODESIC when any fold bailed out. */
int gpt_cf_fullw_sideinfo_folds(int64_t F, const double* const* Rating, const int64_t* N,
                                const double* const* Ratingtest, const int64_t* Ntest,
                                const double* UserData, int64_t n1, int64_t D1,
                                const double* MovieData, int64_t n2, int64_t D2, double signal_var,
                                double sigma_u, double sigma_w, const double* w_init, int64_t r,
                                int64_t m, double epsw, double epsU, double a, double b, double c,
                                int64_t burnin, int64_t maxepoch, uint64_t seed,
                                const double* ytrainMean, const double* ytrainStd,
                                int32_t langevin, int32_t stiefel, int32_t avg,
                                double* const* w_store, double* const* U_store,
                                double* const* V_store, double* const* testpred_store,
                                double* const* trainRMSE, double* const* testRMSE, int32_t* status);

/* Device time of the last CF SGD / SGLD run (any gpt_cf_* SGD entry, fixw / sideinfo / folds)
 * on the calling thread: hipEvents around each epoch launch (cf_epoch_kernel, every live fold's
 * minibatch steps of one epoch) and each evaluation launch (cf_eval_kernel); epochs = epoch
 * launches, fold_steps = minibatch steps summed over the folds live in each launch.  No
 * reference counterpart (measurement, bench.py --workload movielens). */
int gpt_cf_last_timing(double* epoch_ms, double* eval_ms, int64_t* epochs, int64_t* fold_steps);
/* How the last CF SGD / SGLD call on this thread launched its epochs: 0 = per minibatch a
 * batch-phase launch (one workgroup per fold) and a row-parallel move launch; 1 = one launch per
 * epoch with the Stiefel move inside (stiefel = 1); 2 = one launch per epoch with the lazy SGD
 * move (langevin = stiefel = 0 on the feature-mask path: rows outside a batch only decay, read as
 * m·c^Δ).  No reference counterpart (measurement). */
int gpt_cf_last_mode(int32_t* mode);
/* With GPTSGLD_CF_STAMPS set, the last CF SGD call recorded s_memtime at the 8 phase boundaries
 * of fold 0's first 64 steps of its first epoch (batch load, masks / links, sums, sum·w,
 * residuals, gradients, U / V moves): copies up to cap of them (64 x 8, step-major) and returns
 * how many there are (0 without the variable).  Diagnostics. */
int64_t gpt_cf_last_stamps(int64_t* out, int64_t cap);

/* The other SGD / SGLD variants of the CF model (same Rating / Ratingtest / output conventions
 * as gpt_cf_fullw_sideinfo; the NaN bail-out zeroes the parameter stores):
 *   GPT_fixw_sideinfo(Rating,UserData,MovieData,Ratingtest,signal_var,sigma_u,w,m,epsU,a,b,c,
 *     burnin,maxepoch,param_seed,ytrainMean,ytrainStd;langevin,stiefel,avg)
 *     100k_movielensExperiment.jl:282-404 — w fixed, U,V = sigma_u*randn (also when stiefel);
 *     returns U_store (n1+D1,r,T), V_store, testpred_store, trainRMSE, testRMSE.
 *   GPT_fullw(Rating,UserData,MovieData,Ratingtest,signal_var,sigma_u,sigma_w,w_init,m,epsw,epsU,
 *     burnin,maxepoch,param_seed,ytrainMean,ytrainStd;langevin,stiefel,avg)
 *     :160-279 — no side information (pred = sum((U[user,:]*w).*V[movie,:])), U,V = randn or
 *     the Stiefel polar init; returns w_store (r,r,T), U_store (n1,r,T), V_store (n2,r,T), ...
 *   GPT_fixw(Rating,UserData,MovieData,Ratingtest,signal_var,sigma_u,w,m,epsU,burnin,maxepoch,
 *     param_seed,ytrainMean,ytrainStd;langevin,stiefel,avg)
 *     :56-156 — no side information, w fixed, U,V = sigma_u*randn; returns U_store (n1,r,T), ...
 * (The reference's bail-out of GPT_fullw / GPT_fixw returns a 3-tuple of zero arrays; these
 * entry points keep the normal outputs with zeroed parameter stores and GPT_ERR_NAN_GEODESIC.) */
int gpt_cf_fixw_sideinfo(const double* Rating, int64_t N, int64_t ldr, const double* UserData,
                         int64_t n1, int64_t D1, const double* MovieData, int64_t n2, int64_t D2,
                         const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var,
                         double sigma_u, const double* w, int64_t r, int64_t m, double epsU,
                         double a, double b, double c, int64_t burnin, int64_t maxepoch,
                         uint64_t seed, double ytrainMean, double ytrainStd, int32_t langevin,
                         int32_t stiefel, int32_t avg, double* U_store, double* V_store,
                         double* testpred_store, double* trainRMSE, double* testRMSE);
int gpt_cf_fullw(const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
                 const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var,
                 double sigma_u, double sigma_w, const double* w_init, int64_t r, int64_t m,
                 double epsw, double epsU, int64_t burnin, int64_t maxepoch, uint64_t seed,
                 double ytrainMean, double ytrainStd, int32_t langevin, int32_t stiefel,
                 int32_t avg, double* w_store, double* U_store, double* V_store,
                 double* testpred_store, double* trainRMSE, double* testRMSE);
int gpt_cf_fixw(const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
                const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var,
                double sigma_u, const double* w, int64_t r, int64_t m, double epsU, int64_t burnin,
                int64_t maxepoch, uint64_t seed, double ytrainMean, double ytrainStd,
                int32_t langevin, int32_t stiefel, int32_t avg, double* U_store, double* V_store,
                double* testpred_store, double* trainRMSE, double* testRMSE);

/* GPT_fixw_gibbs(Rating,UserData,MovieData,Ratingtest,signal_var,sigma_u,w,burnin,maxepoch,
 *   n_samples,param_seed;avg,rotated_w)  100k_movielensExperiment.jl:945-1028: the user / movie
 * Gibbs conditionals of gpt_cf_fullw_gibbs with w fixed (no w draw); returns U_store (n1,r,T),
 * V_store (n2,r,T), testpred_store, trainRMSE, testRMSE. */
int gpt_cf_fixw_gibbs(const double* Rating, int64_t N, int64_t ldr, int64_t n1, int64_t n2,
                      const double* Ratingtest, int64_t Ntest, int64_t ldt, double signal_var,
                      double sigma_u, const double* w, int64_t r, int64_t burnin,
                      int64_t maxepoch, int64_t n_samples, uint64_t seed, double ytrainMean,
                      double ytrainStd, int32_t avg, int32_t rotated_w, double* U_store,
                      double* V_store, double* testpred_store, double* trainRMSE,
                      double* testRMSE);

/* randperm(N) + phi = phi[:,:,perm] of GPT_SGLD.jl:373-374 for `epochs` epochs of one chain,
 * built on the device by the sessions' own kernel: out (N, epochs) column-major, 0-based rows
 * of the composed order (order_e = order_{e-1}[perm_e]). */
int gpt_epoch_orders(int64_t N, uint64_t seed, int64_t epochs, int32_t* out);

const char* gpt_last_error(void);
/* LDS bytes one step workgroup needs for this shape (must be <= 163840). */
int64_t gpt_sgld_lds_bytes(int64_t n, int64_t D, int64_t r, int64_t Q, int64_t m);
int gpt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* GPTSGLD_H */
