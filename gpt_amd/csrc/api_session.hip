// The device session of the sampler (gpt_sgld_session_*): per-chain state, engine choice, the
// enqueue of steps and their captured graphs, and the gpt_debug_* test entries.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "host_util.h"

using namespace gpt;

// ====================================================================== session
struct gpt_sgld_session {
  gpt_sgld_config cfg{};
  int nchains = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  StepParams P{};
  long long numbatches = 0, total_steps = 0, steps_done = 0, nstore = 0;
  int epochs = 0;
  DevMem I0, chains_d, tbase, status;
  DevSet chain_mem;
  std::vector<ChainDesc> chains_h;
  bool temp_ready = false;
  // Captured step sequences, keyed by where they start in an epoch (b0 = first step % numbatches,
  // which fixes where the epoch-order builds sit) and their length.  A replay reads the step
  // counter from the device, so one graph serves every epoch.
  struct GraphEnt { long long b0; int len; hipGraph_t g; hipGraphExec_t x; };
  std::vector<GraphEnt> graphs;
  bool ran = false;                   // a step has been enqueued (RMSprop must be set before)
  int graph_steps = 0;                // canonical chunk: one epoch (<= 512 steps)
  DevMem ord_ws;                      // epoch-order workspace when a shuffle exceeds LDS
  bool store = false, diag = false;
  int engine = 0;                     // kEngineGrid / kEngineChain / kEngineWave
  DevMem runq;
  DevMem wvtab;                       // wave engine: run members and starts (wave_tables)
  DevMem vtab;                        // grid engine: vphase_cols tables
  // Bounded in-flight work (gpt_sgld_session_run): an event after every chunk it enqueues, and
  // before the chunk that would put more than max_inflight chunks (<= one epoch each) in the
  // stream, a wait for the oldest.  A 200-epoch run() used to enqueue all 200 epoch graphs
  // (80 000 kernel dispatches on the wave engine) before the first finished.
  int max_inflight = 8;               // GPTSGLD_MAX_INFLIGHT; 0 = unbounded
  std::vector<hipEvent_t> inflight;
  long long chunks_enqueued = 0;
  // X mode (gpt_sgld_session_create_x): chains_d keeps the real order rings and targets (the
  // epoch-order kernel and the stager use it, its phi is null); the engines run on view_d, whose
  // phi / y / order are the chain's feature ring, target ring and order view (StageParams).
  bool xmode = false, x_primed = false;
  int xspan = 1;                      // steps per launch at most; the ring holds xspan + 1 batches
  StageParams S{};
  DevMem view_d, xcoef;
  std::vector<ChainDesc> view_h;
  long long stage_bytes = 0;          // ring + view bytes per chain (gpt_sgld_session_staging)

  // Destroy every captured graph (after the stream has drained: a launched graph may still run).
  void drop_graphs() {
    if (graphs.empty()) return;
    (void)hipStreamSynchronize(stream);
    for (auto& g : graphs) {
      (void)hipGraphExecDestroy(g.x);
      (void)hipGraphDestroy(g.g);
    }
    graphs.clear();
  }
  // Also the end of a creation that failed midway: the stream has drained before the members
  // free the device memory.
  ~gpt_sgld_session() {
    if (stream) (void)hipStreamSynchronize(stream);
    drop_graphs();
    for (auto e : inflight) if (e) (void)hipEventDestroy(e);
    if (own_stream) (void)hipStreamDestroy(stream);
  }
};

// The ChainDesc array the step engines read.
static const ChainDesc* engine_chains(const gpt_sgld_session* s) {
  return s->xmode ? s->view_d.as<ChainDesc>() : s->chains_d.as<ChainDesc>();
}

// Engine choice: kFlagGrid (or kFlagWonly / kFlagCls, w-only steps / classification) forces the grid
// engine (sgld.hip), kFlagChain the chain engine (chain.hip), kFlagWave the wave engine (wave.hip);
// otherwise GPTSGLD_ENGINE=grid|chain|wave; otherwise the chain engine whenever it supports the
// shape, else the wave engine (ranks past the chain engine), else the grid engine.  Few chains
// of a chain-engine shape go to the grid engine (D+1 workgroups per chain: the shorter step) as
// long as every chain's workgroups fit the GPU at once.  (Engine 2, the round-3 split engine —
// the grid engine with the batch in slices and an in-kernel barrier — measured slower at every
// slice count and was removed in round 4; kFlagSplit / "split" are rejected.)  Every error here is
// one of the arguments and comes before the first HIP call; only the automatic choice asks the
// device, for its CU count.
static int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return cus;
}

static int pick_engine(const gpt_sgld_config* c, const int32_t* I_host, int32_t flags,
                       int nchains, int* engine) {
  int max_run = 0;                    // longest run of core entries sharing one I[·,k] value
  for (int k = 0; k < (int)c->D; ++k) {
    std::vector<int> cnt((size_t)c->r + 1, 0);
    for (int q = 0; q < (int)c->Q; ++q) max_run = std::max(max_run, ++cnt[I_host[q + c->Q * k]]);
  }
  const bool chain_ok = chain_supported((int)c->n, (int)c->D, (int)c->r, (int)c->Q, (int)c->m,
                                        c->langevin != 0, c->stiefel != 0, max_run);
  const bool grid_ok =
      step_layout((int)c->n, (int)c->D, (int)c->r, (int)c->Q, (int)c->m).bytes <= kMaxLds;
  const bool wave_ok = wave_supported((int)c->n, (int)c->D, (int)c->r, (int)c->Q, (int)c->m,
                                      c->langevin != 0, c->stiefel != 0);
  if (flags & kFlagSplit) { set_error("the split engine (store_flags bit 6) was removed"); return GPT_ERR_BAD_DIMS; }
  // explicit store_flags win over the environment: RMSprop-capable sessions, w-only steps and
  // classification exist only on the grid engine
  int want = -1;
  if (flags & (kFlagGrid | kFlagWonly | kFlagCls)) want = kEngineGrid;
  else if (flags & kFlagChain) want = kEngineChain;
  else if (flags & kFlagWave) want = kEngineWave;
  else if (const char* ev = std::getenv("GPTSGLD_ENGINE")) {
    if (!std::strcmp(ev, "grid")) want = kEngineGrid;
    else if (!std::strcmp(ev, "chain")) want = kEngineChain;
    else if (!std::strcmp(ev, "split")) {
      set_error("the split engine (GPTSGLD_ENGINE=split) was removed"); return GPT_ERR_BAD_DIMS;
    }
    else if (!std::strcmp(ev, "wave")) want = kEngineWave;
  }
  if (want == kEngineWave && !wave_ok) {
    set_error("wave engine does not support this shape (needs SGLD+Stiefel, r in {6,8,10,12,15,"
              "16,20}, 3r <= n <= 256, m <= 64, the V-phase working set within 160 KiB LDS)");
    return GPT_ERR_BAD_DIMS;
  }
  if (want == kEngineChain && !chain_ok) {
    set_error("chain engine does not support this shape (needs D<=8, r<=5, n<=512 (even if >64), "
              "Q<=256, SGLD+Stiefel, <=64 core entries per I[.,k] value)");
    return GPT_ERR_BAD_DIMS;
  }
  if (want == kEngineGrid && !grid_ok) {
    set_error("grid engine: working set exceeds 160 KiB LDS"); return GPT_ERR_BAD_DIMS;
  }
  // few chains: the grid engine's D+1 workgroups per chain (the shorter step)
  // ranks past the chain engine: the wave engine (its step is shorter than the grid engine's even
  // for one chain: the geodesic's expm runs on every dimension's wave at once)
  if (want < 0 && !chain_ok && wave_ok) want = kEngineWave;
  if (want < 0 && grid_ok && (long long)nchains * (c->D + 1) <= device_cus()) want = kEngineGrid;
  *engine = want >= 0 ? want : (chain_ok ? kEngineChain : kEngineGrid);
  return GPT_OK;
}

// Chain engine tables: for every dimension k the core entries ordered by (I[q,k], q):
// pos[q + Q*k] = rank of q, seg[k*(r+1) + l] = first rank with I[q,k] = l (0-based).
// Run members of the chain engine's core sums (see gpt_internal.h StepParams::runq).
static void chain_runq(const std::vector<int32_t>& I0, int Q, int D, int r,
                       std::vector<int32_t>& out) {
  out.assign((size_t)D * r * 64, 256);
  for (int k = 0; k < D; ++k) {
    std::vector<int> cnt(r, 0);
    for (int q = 0; q < Q; ++q) {
      const int l = I0[q + (size_t)Q * k];
      out[((size_t)k * r + l) * 64 + cnt[l]++] = q;   // max run <= 64 (chain_supported)
    }
  }
}

// Steps t_local .. t_local+nsteps-1 of the sequence being enqueued (nsteps > 1 only on the chain
// engine, within one epoch: every other kernel is one step per launch).
static hipError_t session_launch(gpt_sgld_session* s, const StepParams& P, int t_local,
                                 int nsteps) {
  if (P.ncls)
    return launch_step_cls(P, engine_chains(s), s->nchains, s->tbase.as<long long>(),
                           t_local, s->stream);
  if (P.wonly)
    return launch_step_wonly(P, engine_chains(s), s->nchains, s->tbase.as<long long>(),
                             t_local, s->stream);
  if (P.rms)
    return launch_step_rms(P, engine_chains(s), s->nchains, s->tbase.as<long long>(),
                           t_local, s->stream);
  if (s->engine == kEngineChain)
    return launch_chain(P, engine_chains(s), s->nchains, s->tbase.as<long long>(),
                        t_local, nsteps, s->stream);
  if (s->engine == kEngineWave)
    return launch_wave(P, engine_chains(s), s->nchains, s->tbase.as<long long>(),
                       t_local, false, s->stream);
  return launch_step(P, engine_chains(s), s->nchains, s->tbase.as<long long>(),
                     t_local, s->stream);
}

// X mode: stage batches tbase[0] + t_first .. + count - 1 into the rings (feature.hip).
static hipError_t session_stage(gpt_sgld_session* s, int t_first, int count) {
  return launch_stage_batches(s->S, s->chains_d.as<ChainDesc>(), s->view_d.as<ChainDesc>(),
                              s->nchains, s->tbase.as<long long>(), t_first, count, s->stream);
}

// temp of the first step (grid engine only: the chain engine forms temp inside its step).  An X
// session stages the batch of its first step here, once, on every engine: from then on each
// launch's stager call leaves the batch after the launch's last step in the ring.
static int session_prime(gpt_sgld_session* s) {
  if (s->xmode && !s->x_primed) {
    const hipError_t e = session_stage(s, 0, 1);
    if (e != hipSuccess) return hip_fail(e, "launch_stage_batches");
    s->x_primed = true;
  }
  if (s->engine == kEngineChain || s->temp_ready) return GPT_OK;
  hipError_t e = s->engine == kEngineWave
                     ? launch_wave(s->P, engine_chains(s), s->nchains,
                                   s->tbase.as<long long>(), 0, true, s->stream)
                     : launch_temp_init(s->P, engine_chains(s), s->nchains,
                                        s->tbase.as<long long>(), s->stream);
  if (e != hipSuccess) return hip_fail(e, "launch_temp_init");
  s->temp_ready = true;
  return GPT_OK;
}

// Before the first step of epoch e, order_{e+1} goes into the ring slot order_{e-1} leaves
// (order.hip).  t_host = the step's index as the host counts it: in a captured sequence only its
// position in the epoch matters (the kernel reads the step counter from the device).
static hipError_t session_epoch_order(gpt_sgld_session* s, long long t_host, int t_local) {
  if (t_host % s->P.nb != 0) return hipSuccess;
  return launch_epoch_order(s->chains_d.as<ChainDesc>(), s->nchains, s->P.N, s->P.nb,
                            s->total_steps, s->tbase.as<long long>(), t_local, -1,
                            s->ord_ws.as<int32_t>(), s->stream);
}

// Steps of one epoch at most that one launch runs from host step t_host (chain engine: the rest of
// the epoch within `left`; other engines: 1).  An X session's launches stop at xspan steps: its
// ring holds the launch's batches and the one after them (session_stage_ahead).
static int session_span(const gpt_sgld_session* s, long long t_host, long long left) {
  if (s->engine != kEngineChain || s->P.rms || s->P.wonly || s->P.ncls) return 1;
  const long long span = std::min<long long>(left, s->P.nb - t_host % s->P.nb);
  return (int)(s->xmode ? std::min<long long>(span, s->xspan) : span);
}

// X mode, before the launch of steps t_local .. t_local+span-1: step t reads batch t and already
// batch t+1 (the wave and grid engines form the next batch's temp at the end of the step, the
// chain engine's next launch starts on it), so batches t_local+1 .. t_local+span go into the ring
// now (batch t_local is there since the launch before, or since session_prime).  The ring's
// span + 1 <= KR slots are all distinct, so no write lands on a slot this launch reads.  Called
// after session_epoch_order: batch t_local+span may open epoch e+1, whose order exists from the
// first step of epoch e on.
static hipError_t session_stage_ahead(gpt_sgld_session* s, int t_local, int span) {
  if (!s->xmode) return hipSuccess;
  return session_stage(s, t_local + 1, span);
}

// The launches of the next `count` steps, of at most max_span steps each, and the advance of the
// device's step counter behind them.  Every launch goes through around(i, launch): i = its first
// step, counted from the sequence's start, and launch(P) enqueues it with the caller's StepParams.
// What around adds sits between the stager and the step kernel, and after it.
template <class Around>
static int session_launches(gpt_sgld_session* s, long long count, int max_span, Around&& around) {
  s->ran = true;
  for (long long i = 0; i < count;) {
    hipError_t e = session_epoch_order(s, s->steps_done + i, (int)i);
    if (e != hipSuccess) return hip_fail(e, "launch_epoch_order");
    const int span = std::min(session_span(s, s->steps_done + i, count - i), max_span);
    e = session_stage_ahead(s, (int)i, span);
    if (e != hipSuccess) return hip_fail(e, "launch_stage_batches");
    GPT_TRY(around(i, [&](const StepParams& P) {
      const hipError_t el = session_launch(s, P, (int)i, span);
      return el == hipSuccess ? GPT_OK : hip_fail(el, "launch_step");
    }));
    i += span;
  }
  const hipError_t e = launch_advance(s->tbase.as<long long>(), count, s->stream);
  return e == hipSuccess ? GPT_OK : hip_fail(e, "launch_advance");
}
constexpr int kAnySpan = 1 << 30;

// The plain sequence (also what a graph captures): nothing around the launches.
static int session_enqueue(gpt_sgld_session* s, int count) {
  return session_launches(s, count, kAnySpan,
                          [&](long long, auto&& launch) { return launch(s->P); });
}

// The inputs an X session keeps in place of per-chain phi (gpt_sgld_session_create_x).
struct XInputs {
  const double* X;                // (N, D) device, shared by the chains
  const double* ls;               // (ls_len, nchains) device
  int ls_len;
  const double* sigma_rbf;        // nchains, host
  double phi_scale;
  const double* Z;                // (n, D) device, shared
  const double* b;                // (n, D) device, shared
};

// The step counts of a configuration: batches per epoch, epochs, steps run and samples stored.
struct SessionCounts { long long nb, total, nstore; int epochs; };
static SessionCounts session_counts(const gpt_sgld_config* c) {
  SessionCounts k{};
  k.nb = (c->N + c->m - 1) / c->m;
  k.epochs = (int)(c->burnin + c->maxepoch);
  k.total = (long long)k.epochs * k.nb;
  if (c->max_steps > 0) k.total = std::min<long long>(k.total, c->max_steps);
  k.nstore = (c->maxepoch * k.nb) / c->store_every;
  return k;
}

// StepParams of the session's configuration (s->P starts zeroed: no RMSprop, no diagnostics
// buffers) and the tables of its engine on the device.
static int session_step_params(gpt_sgld_session* s, const std::vector<int32_t>& I0, int32_t flags) {
  const gpt_sgld_config& c = s->cfg;
  const int n = (int)c.n, D = (int)c.D, r = (int)c.r, Q = (int)c.Q, m = (int)c.m;
  StepParams& P = s->P;
  P.n = n; P.D = D; P.N = (int)c.N; P.r = r; P.Q = Q; P.m = m; P.nb = (int)s->numbatches;
  P.burnin_steps = (int)(c.burnin * s->numbatches);
  P.total_steps = s->total_steps;
  P.store_every = (int)c.store_every;
  P.langevin = c.langevin; P.stiefel = c.stiefel;
  P.wonly = (flags & kFlagWonly) ? 1 : 0;
  P.ncls = (flags & kFlagCls) ? s->nchains : 0;
  GPT_HIPCHK(s->I0.upload(I0.data(), I0.size()));
  P.I0 = s->I0.as<int32_t>();
  if (s->engine == kEngineChain) {
    std::vector<int32_t> rq;
    chain_runq(I0, Q, D, r, rq);
    GPT_HIPCHK(s->runq.upload(rq.data(), rq.size()));
    P.runq = s->runq.as<int32_t>();
  } else if (s->engine == kEngineWave) {
    std::vector<uint16_t> wt;
    wave_tables(I0, Q, D, r, m, wt);
    GPT_HIPCHK(s->wvtab.upload(wt.data(), wt.size()));
    P.wvtab = s->wvtab.as<uint16_t>();
  } else if (step_layout(n, D, r, Q, m).vcols) {
    std::vector<int32_t> vt;
    vphase_cols_tables(I0, n, D, r, Q, m, vt);
    GPT_HIPCHK(s->vtab.upload(vt.data(), vt.size()));
    P.vtab = s->vtab.as<int32_t>();
  }
  return GPT_OK;
}

// X mode: the steps per launch, the stager's parameters (but o_rows: the block layout gives it)
// and the chains' feature scales.
static int session_x_setup(gpt_sgld_session* s, const XInputs& x) {
  const StepParams& P = s->P;
  s->xmode = true;
  s->xspan = s->engine == kEngineChain ? kXSpanCap : 1;
  if (const char* ev = std::getenv("GPTSGLD_XSPAN")) {   // measurement (scripts/time_xmode.py)
    const int v = std::atoi(ev);
    if (s->engine == kEngineChain && (v == 4 || v == 8 || v == 16)) s->xspan = v;
  }
  const size_t KR = (size_t)s->xspan + 1;
  s->stage_bytes = (long long)(KR * P.m * (8 * (size_t)P.n * P.D + 8 + 4) + 4 * 2 * (size_t)P.N);
  StageParams& S = s->S;
  S.X = x.X; S.Z = x.Z; S.b = x.b; S.ls = x.ls; S.ls_len = x.ls_len;
  S.N = P.N; S.n = P.n; S.D = P.D; S.m = P.m; S.nb = P.nb; S.KR = (int)KR;
  S.total_steps = s->total_steps;
  std::vector<double> cf(s->nchains);                    // c of gpt_feature, per chain
  for (int c = 0; c < s->nchains; ++c)
    cf[c] = x.phi_scale * std::pow(x.sigma_rbf[c], 1.0 / (double)P.D) * std::sqrt(2.0 / (double)P.n);
  GPT_HIPCHK(s->xcoef.upload(cf.data(), cf.size()));
  S.cfeat = s->xcoef.as<double>();
  s->view_h.resize(s->nchains);
  return GPT_OK;
}

// A chain's device block, one allocation: the arrays of its descriptor in this order, each on a
// 256-byte boundary.  X mode appends the feature ring (KR batch slots of m rows: the chain
// engine's LDS-DMA takes 16-byte pieces), the target ring, the staged row numbers and the order
// view; the three the engines read come back in ring.phi / .y / .order.  Returned: the byte
// offsets at which the parts that session_init_chain zero-fills begin.
struct ChainSpans { size_t stores, diag, wave, x, rows, end; };
static ChainSpans carve_chain(Carve& k, const gpt_sgld_session& s, ChainDesc& C, ChainDesc& ring) {
  const StepParams& P = s.P;
  const size_t Q = P.Q, N = P.N, nrD = (size_t)P.n * P.r * P.D, Drm = (size_t)P.D * P.r * P.m;
  const bool wave = s.engine == kEngineWave;
  ChainSpans o{};
  C.w = k.take<double>(2 * Q);
  C.U = k.take<double>(nrD);
  C.temp = k.take<double>(2 * Drm);
  C.order = k.take<int32_t>(2 * N);
  o.stores = k.off;
  C.w_store = s.store ? k.take<double>(Q * s.nstore) : nullptr;
  C.U_store = s.store ? k.take<double>(nrD * s.nstore) : nullptr;
  o.diag = k.off;
  C.diag = s.diag ? k.take<double>((size_t)(1 + P.D) * s.total_steps) : nullptr;
  o.wave = k.off;
  C.coef = wave ? k.take<double>(Drm) : nullptr;
  C.park = wave ? k.take<double>(nrD) : nullptr;
  o.x = o.rows = k.off;
  if (s.xmode) {
    const size_t rows = (size_t)s.S.KR * P.m;
    ring.phi = k.take<double>(rows * P.n * P.D);
    ring.y = k.take<double>(rows);
    o.rows = k.off;
    k.take<int32_t>(rows);
    ring.order = k.take<int32_t>(2 * N);
  }
  o.end = k.off;
  return o;
}

// Chain c's hyper-parameters, in its descriptor and in the X view's copy of it.
static void chain_set_hyper(gpt_sgld_session* s, int c, double epsw, double epsU,
                            double signal_var, double sigma_w) {
  for (std::vector<ChainDesc>* v : {&s->chains_h, &s->view_h}) {
    if (v->empty()) continue;
    ChainDesc& C = (*v)[c];
    C.epsw = epsw; C.epsU = epsU; C.signal_var = signal_var; C.sigma_w = sigma_w;
  }
}

// Chain c of a new session: its block (laid out as `o` counted it), the descriptor and the X view
// on the host, the initial state, and zeros where a kernel adds to or may read before it writes.
static int session_init_chain(gpt_sgld_session* s, int c, const ChainSpans& o, const double* phi,
                              const double* y, uint64_t seed, std::vector<double>& w0,
                              std::vector<double>& U0) {
  const gpt_sgld_config& cfg = s->cfg;
  Carve k;
  GPT_HIPCHK(s->chain_mem.alloc(&k.base, o.end));
  ChainDesc& C = s->chains_h[c];
  ChainDesc ring{};
  carve_chain(k, *s, C, ring);
  C.phi = phi;
  C.y = y;
  C.status = s->status.as<int32_t>() + c;
  C.seed = seed;
  if (s->xmode) {
    ChainDesc& V = s->view_h[c];
    V = C;
    V.phi = ring.phi; V.y = ring.y; V.order = ring.order;
  }
  chain_set_hyper(s, c, cfg.epsw, cfg.epsU, cfg.signal_var, cfg.sigma_w);
  host_init_state((int)cfg.n, (int)cfg.r, (int)cfg.D, (int)cfg.Q, seed, cfg.stiefel != 0,
                  cfg.sigma_w, w0.data(), U0.data());
  GPT_HIPCHK(hipMemcpy(C.w, w0.data(), 8 * w0.size(), hipMemcpyHostToDevice));
  GPT_HIPCHK(hipMemcpy(C.U, U0.data(), 8 * U0.size(), hipMemcpyHostToDevice));
  if (s->store) GPT_HIPCHK(hipMemset(k.base + o.stores, 0, o.diag - o.stores));
  if (s->diag) GPT_HIPCHK(hipMemset(k.base + o.diag, 0, o.wave - o.diag));
  // every view entry is a ring row at all times: a read the engines discard stays in the ring
  if (s->xmode) GPT_HIPCHK(hipMemset(k.base + o.x, 0, o.end - o.x));
  return GPT_OK;
}

// A phi session (phi_dev, xin null) or an X session (xin, phi_dev null).
static int session_create(const gpt_sgld_config* cfg, int32_t nchains, const uint64_t* seeds,
                          const double* const* phi_dev, const double* const* y_dev,
                          const int32_t* I_host, int32_t store_flags, void* hip_stream,
                          const XInputs* xin, gpt_sgld_session** out) {
  if (!out) { set_error("null out"); return GPT_ERR_BAD_DIMS; }
  *out = nullptr;
  // what needs no device: the configuration, the chain arguments, I, the engine asked for
  if (!valid_cfg(cfg)) return GPT_ERR_BAD_DIMS;
  if (nchains < 1 || !seeds || (!phi_dev && !xin) || !y_dev || !I_host) {
    set_error("bad chain arguments"); return GPT_ERR_BAD_DIMS;
  }
  std::vector<int32_t> I0;
  if (!zero_based_I(I_host, cfg->Q, cfg->D, cfg->r, I0)) return GPT_ERR_BAD_DIMS;
  int engine = 0;
  GPT_TRY(pick_engine(cfg, I_host, store_flags, nchains, &engine));
  const hipError_t he = set_lds_limits();
  if (he != hipSuccess) return hip_fail(he, "hipFuncSetAttribute");

  std::unique_ptr<gpt_sgld_session> s(new gpt_sgld_session());
  const SessionCounts cnt = session_counts(cfg);
  s->cfg = *cfg;
  s->nchains = nchains;
  s->engine = engine;
  s->numbatches = cnt.nb; s->epochs = cnt.epochs; s->total_steps = cnt.total; s->nstore = cnt.nstore;
  s->store = (store_flags & kFlagStore) != 0;
  s->diag = (store_flags & kFlagDiag) != 0;
  if (hip_stream) s->stream = (hipStream_t)hip_stream;
  else {
    GPT_HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->own_stream = true;
  }
  GPT_TRY(session_step_params(s.get(), I0, store_flags));
  GPT_HIPCHK(s->tbase.alloc<long long>(1));
  GPT_HIPCHK(s->tbase.zero());
  GPT_HIPCHK(s->status.alloc<int32_t>(nchains));
  GPT_HIPCHK(s->status.zero());
  if (xin) GPT_TRY(session_x_setup(s.get(), *xin));

  // one allocation per chain: the layout is counted once, then handed out chain by chain
  Carve count;
  ChainDesc unused{};
  const ChainSpans o = carve_chain(count, *s, unused, unused);
  s->S.o_rows = o.rows - o.x;
  std::vector<double> w0((size_t)cfg->Q), U0((size_t)(cfg->n * cfg->r * cfg->D));
  s->chains_h.resize(nchains);
  for (int c = 0; c < nchains; ++c)
    GPT_TRY(session_init_chain(s.get(), c, o, xin ? nullptr : phi_dev[c], y_dev[c], seeds[c], w0, U0));
  GPT_HIPCHK(s->chains_d.upload(s->chains_h.data(), s->chains_h.size()));
  if (xin) GPT_HIPCHK(s->view_d.upload(s->view_h.data(), s->view_h.size()));
  // order_0 of every chain (the first step builds order_1, session_epoch_order)
  const int N = (int)cfg->N;
  if (const size_t wsi = epoch_order_ws_ints(N, nchains)) GPT_HIPCHK(s->ord_ws.alloc<int32_t>(wsi));
  GPT_HIPCHK(launch_epoch_order(s->chains_d.as<ChainDesc>(), nchains, N, (int)s->numbatches,
                                s->total_steps, s->tbase.as<long long>(), 0, 0,
                                s->ord_ws.as<int32_t>(), s->stream));
  // (an X session's epoch graph holds several chain launches of at most xspan steps, each behind
  // its stager call: session_span cuts them, session_next_chunk and the graph keys do not change)
  s->graph_steps = (int)std::min<long long>(std::max<long long>(s->numbatches, 1), 512);
  if (const char* ev = std::getenv("GPTSGLD_MAX_INFLIGHT")) s->max_inflight = std::max(0, std::atoi(ev));
  *out = s.release();
  return GPT_OK;
}

extern "C" int gpt_sgld_session_create(const gpt_sgld_config* cfg, int32_t nchains,
                                       const uint64_t* seeds, const double* const* phi_dev,
                                       const double* const* y_dev, const int32_t* I_host,
                                       int32_t store_flags, void* hip_stream,
                                       gpt_sgld_session** out) {
  if (out) *out = nullptr;
  if (!phi_dev) { set_error("bad chain arguments"); return GPT_ERR_BAD_DIMS; }
  return session_create(cfg, nchains, seeds, phi_dev, y_dev, I_host, store_flags, hip_stream,
                        nullptr, out);
}

extern "C" int gpt_sgld_session_create_x(const gpt_sgld_config* cfg, int32_t nchains,
                                         const uint64_t* seeds, const double* X_dev,
                                         const double* const* y_dev, const double* ls_dev,
                                         int64_t ls_len, const double* sigma_rbf, double phi_scale,
                                         const double* Z_dev, const double* b_dev,
                                         const int32_t* I_host, int32_t store_flags,
                                         void* hip_stream, gpt_sgld_session** out) {
  if (!out) { set_error("null out"); return GPT_ERR_BAD_DIMS; }
  *out = nullptr;
  if (!valid_x_args(cfg, nchains, seeds, X_dev, y_dev, ls_dev, ls_len, sigma_rbf, Z_dev, b_dev,
                    I_host, store_flags))
    return GPT_ERR_BAD_DIMS;
  const XInputs xin{X_dev, ls_dev, (int)ls_len, sigma_rbf, phi_scale, Z_dev, b_dev};
  return session_create(cfg, nchains, seeds, nullptr, y_dev, I_host, store_flags, hip_stream, &xin,
                        out);
}

extern "C" int gpt_sgld_session_staging(gpt_sgld_session* s, int64_t* out) {
  if (!s || !out) { set_error("null argument"); return GPT_ERR_BAD_DIMS; }
  out[0] = s->xmode ? s->S.KR : 0;
  out[1] = s->stage_bytes;
  out[2] = s->xmode ? 1 : 0;
  return GPT_OK;
}

namespace gpt {

// Every check of an X session's arguments that needs no device (also the host-array form's).
bool valid_x_args(const gpt_sgld_config* cfg, int32_t nchains, const uint64_t* seeds,
                  const double* X, const double* const* y, const double* ls, int64_t ls_len,
                  const double* sigma_rbf, const double* Z, const double* b, const int32_t* I,
                  int32_t store_flags) {
  if (!valid_cfg(cfg)) return false;
  if (nchains < 1 || nchains > 65535) { set_error("X mode: 1 <= nchains <= 65535"); return false; }
  if (!seeds || !X || !y || !ls || !sigma_rbf || !Z || !b || !I) {
    set_error("X mode: null argument"); return false;
  }
  if (ls_len != 1 && ls_len != cfg->D) {
    set_error("dimensions of X and length_scale do not match"); return false;
  }
  for (int c = 0; c < nchains; ++c)
    if (!y[c]) { set_error("X mode: null per-chain y"); return false; }
  if (store_flags & ~(kFlagStore | kFlagDiag | kFlagGrid | kFlagChain | kFlagWave)) {
    set_error("X mode runs the regression steps of the grid, chain and wave engines (store_flags "
              "bits 2, 3, 7): no w-only, classification or split-engine sessions");
    return false;
  }
  return true;
}

// Overwrite chain c's initial state (w_init/U_init injection of the host API).  On the Stiefel
// path the kernels take geod's A = Uᵀmom as (M − Mᵀ)/2 (and the grid engine S from the Gram
// identity), which holds only for UᵀU = I: a U_init off the manifold is rejected.
int session_set_state(gpt_sgld_session* s, int c, const double* w, const double* U) {
  const ChainDesc& C = s->chains_h[c];
  if (U && s->cfg.stiefel) {
    const int n = s->P.n, r = s->P.r, D = s->P.D;
    for (int k = 0; k < D; ++k) {
      const double* Uk = U + (size_t)n * r * k;
      for (int a = 0; a < r; ++a)
        for (int b = a; b < r; ++b) {
          double g = 0.0;
          for (int j = 0; j < n; ++j) g += Uk[j + (size_t)n * a] * Uk[j + (size_t)n * b];
          if (std::fabs(g - (a == b ? 1.0 : 0.0)) > 1e-10) {
            set_error("U_init must have orthonormal columns in every dimension (max |U_kᵀU_k - I| "
                      "<= 1e-10) on the Stiefel path");
            return GPT_ERR_BAD_DIMS;
          }
        }
    }
  }
  if (w) GPT_HIPCHK(hipMemcpy(C.w, w, 8 * (size_t)s->P.Q, hipMemcpyHostToDevice));
  if (U) GPT_HIPCHK(hipMemcpy(C.U, U, 8 * (size_t)s->P.n * s->P.r * s->P.D, hipMemcpyHostToDevice));
  s->temp_ready = false;
  return GPT_OK;
}

// Per-chain zeroed gw (Q) | gU (n·r·D) | res (m) buffers of the RMSprop and classification steps.
int session_alloc_aux(gpt_sgld_session* s) {
  const StepParams& P = s->P;
  const size_t nq = (size_t)P.Q, nu = (size_t)P.n * P.r * P.D;
  for (int c = 0; c < s->nchains; ++c) {
    ChainDesc& C = s->chains_h[c];
    GPT_HIPCHK(s->chain_mem.alloc(&C.gw, nq + nu + (size_t)P.m));
    GPT_HIPCHK(s->chain_mem.mem.back().zero());
    C.gU = C.gw + nq;
    C.res = C.gU + nu;
  }
  GPT_HIPCHK(hipMemcpy(s->chains_d.p, s->chains_h.data(), sizeof(ChainDesc) * s->nchains,
                       hipMemcpyHostToDevice));
  return GPT_OK;
}

SessionRun session_run_info(const gpt_sgld_session* s) {
  return SessionRun{s->total_steps, s->nstore, s->chains_h[0].U};
}

}  // namespace gpt

extern "C" int gpt_sgld_session_set_hyper(gpt_sgld_session* s, int32_t chain, double epsw,
                                          double epsU, double signal_var, double sigma_w) {
  if (!s || chain < 0 || chain >= s->nchains) { set_error("bad chain"); return GPT_ERR_BAD_DIMS; }
  if (!(signal_var > 0) || !(sigma_w > 0)) { set_error("variances must be > 0"); return GPT_ERR_BAD_DIMS; }
  chain_set_hyper(s, chain, epsw, epsU, signal_var, sigma_w);
  GPT_HIPCHK(hipMemcpy(s->chains_d.as<ChainDesc>() + chain, &s->chains_h[chain], sizeof(ChainDesc),
                       hipMemcpyHostToDevice));
  if (s->xmode)                            // the engines read the view's copy
    GPT_HIPCHK(hipMemcpy(s->view_d.as<ChainDesc>() + chain, &s->view_h[chain], sizeof(ChainDesc),
                         hipMemcpyHostToDevice));
  return GPT_OK;
}

extern "C" int gpt_sgld_session_set_rmsprop(gpt_sgld_session* s, double epsilon, double alpha) {
  if (!s) { set_error("null session"); return GPT_ERR_BAD_DIMS; }
  if (s->xmode) { set_error("RMSprop steps are not available on an X session"); return GPT_ERR_BAD_DIMS; }
  if (s->engine != kEngineGrid) {
    set_error("RMSprop steps run on the grid engine: create the session with store_flags bit 2");
    return GPT_ERR_BAD_DIMS;
  }
  if (!s->cfg.stiefel || !s->cfg.langevin) {
    set_error("GPT_SGLDERM_RMSprop is the SGLD + Stiefel sampler (langevin = stiefel = 1)");
    return GPT_ERR_BAD_DIMS;
  }
  if (s->steps_done != 0 || s->ran) { set_error("set RMSprop before the first run"); return GPT_ERR_BAD_DIMS; }
  if (!(epsilon > 0) || !(alpha >= 0 && alpha < 1)) {
    set_error("RMSprop needs epsilon > 0 and 0 <= alpha < 1"); return GPT_ERR_BAD_DIMS;
  }
  GPT_TRY(session_alloc_aux(s));           // moving averages start at 0 (:1143-1144)
  s->P.rms = 1; s->P.rms_eps = epsilon; s->P.rms_alpha = alpha;
  // graphs prepared before this call (gpt_sgld_session_prepare) captured plain SGLD steps: drop
  // them so the next run captures RMSprop steps
  s->drop_graphs();
  return GPT_OK;
}

// The graph replaying `len` steps from a start at b0 = step % numbatches (captured on first use).
static int session_graph(gpt_sgld_session* s, int len, hipGraphExec_t* out) {
  const long long b0 = s->steps_done % s->P.nb;
  for (auto& g : s->graphs)
    if (g.b0 == b0 && g.len == len) { *out = g.x; return GPT_OK; }
  if (s->graphs.size() >= 16) {                // bounded cache: drop the oldest
    GPT_HIPCHK(hipStreamSynchronize(s->stream));   // it may still be running (launches are async)
    (void)hipGraphExecDestroy(s->graphs.front().x);
    (void)hipGraphDestroy(s->graphs.front().g);
    s->graphs.erase(s->graphs.begin());
  }
  GPT_HIPCHK(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
  int rc = session_enqueue(s, len);
  hipGraph_t g = nullptr;
  hipError_t ee = hipStreamEndCapture(s->stream, &g);
  if (rc != GPT_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (ee != hipSuccess) return hip_fail(ee, "hipStreamEndCapture");
  hipGraphExec_t x = nullptr;
  ee = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
  if (ee != hipSuccess) { (void)hipGraphDestroy(g); return hip_fail(ee, "hipGraphInstantiate"); }
  s->graphs.push_back({b0, len, g, x});
  // upload now (ordered on the session stream), so a graph prepared ahead of a timed region does
  // not pay its first-launch upload inside it
  GPT_HIPCHK(hipGraphUpload(x, s->stream));
  *out = x;
  return GPT_OK;
}

// Chunks of a run of n steps from the current step: up to the end of the current epoch, then whole
// epochs (graph_steps), then the remainder.
static int session_next_chunk(const gpt_sgld_session* s, long long remaining, long long at) {
  const long long to_epoch_end = s->graph_steps - (at % s->P.nb) % s->graph_steps;
  return (int)std::min<long long>(remaining, to_epoch_end);
}

// Before enqueueing a chunk: wait until fewer than max_inflight chunks are outstanding.
static int session_throttle(gpt_sgld_session* s) {
  if (s->max_inflight <= 0) return GPT_OK;
  if (s->inflight.empty()) {
    s->inflight.assign(s->max_inflight, nullptr);
    for (auto& e : s->inflight) GPT_HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  if (s->chunks_enqueued >= s->max_inflight)
    GPT_HIPCHK(hipEventSynchronize(s->inflight[s->chunks_enqueued % s->max_inflight]));
  return GPT_OK;
}

// After enqueueing a chunk: mark its end in the ring slot the throttle waits on later.
static int session_mark(gpt_sgld_session* s) {
  if (s->max_inflight <= 0) return GPT_OK;
  GPT_HIPCHK(hipEventRecord(s->inflight[s->chunks_enqueued % s->max_inflight], s->stream));
  ++s->chunks_enqueued;
  return GPT_OK;
}

extern "C" int gpt_sgld_session_run(gpt_sgld_session* s, int64_t nsteps) {
  if (!s) { set_error("null session"); return GPT_ERR_BAD_DIMS; }
  long long remaining = std::min<long long>(nsteps, s->total_steps - s->steps_done);
  if (remaining <= 0) return GPT_OK;
  GPT_TRY(session_prime(s));
  while (remaining > 0) {
    GPT_TRY(session_throttle(s));
    const int chunk = session_next_chunk(s, remaining, s->steps_done);
    // a whole canonical chunk, or any chunk prepared beforehand (gpt_sgld_session_prepare), runs as
    // one graph; other partial chunks are launched directly
    const long long b0 = s->steps_done % s->P.nb;
    bool cached = false;
    for (auto& g : s->graphs) cached |= (g.b0 == b0 && g.len == chunk);
    if (chunk == s->graph_steps || cached) {
      hipGraphExec_t x = nullptr;
      GPT_TRY(session_graph(s, chunk, &x));
      GPT_HIPCHK(hipGraphLaunch(x, s->stream));
      s->ran = true;
    } else {
      GPT_TRY(session_enqueue(s, chunk));
    }
    s->steps_done += chunk;
    remaining -= chunk;
    GPT_TRY(session_mark(s));
  }
  return GPT_OK;
}

extern "C" int gpt_sgld_session_prepare(gpt_sgld_session* s, int64_t nsteps) {
  if (!s) { set_error("null session"); return GPT_ERR_BAD_DIMS; }
  long long remaining = std::min<long long>(nsteps, s->total_steps - s->steps_done);
  const long long saved = s->steps_done;
  const bool ran = s->ran;
  int rc = GPT_OK;
  while (remaining > 0 && rc == GPT_OK) {  // the same chunking as gpt_sgld_session_run
    const int chunk = session_next_chunk(s, remaining, s->steps_done);
    hipGraphExec_t x = nullptr;
    rc = session_graph(s, chunk, &x);
    s->steps_done += chunk;
    remaining -= chunk;
  }
  s->steps_done = saved;                   // capture enqueues nothing: the position is unchanged
  s->ran = ran;
  return rc;
}

extern "C" int gpt_sgld_session_time_steps(gpt_sgld_session* s, int64_t nsteps, double* avg_us) {
  if (!s) { set_error("null session"); return GPT_ERR_BAD_DIMS; }
  const long long cnt = std::min<long long>(nsteps, s->total_steps - s->steps_done);
  if (avg_us) *avg_us = 0.0;
  if (cnt <= 0) return GPT_OK;
  GPT_TRY(session_prime(s));
  ScopedEvents evs;
  GPT_HIPCHK(evs.create(2 * cnt));
  std::vector<hipEvent_t>& ev = evs.e;
  // one event pair per launch (a launch runs `span` steps on the chain engine), around the step
  // kernel alone: the epoch order and the stager's call stay outside it
  long long nl = 0;
  const int rc = session_launches(s, cnt, kAnySpan, [&](long long, auto&& launch) {
    GPT_HIPCHK(hipEventRecord(ev[2 * nl], s->stream));
    GPT_TRY(launch(s->P));
    GPT_HIPCHK(hipEventRecord(ev[2 * nl + 1], s->stream));
    ++nl;
    return (int)GPT_OK;
  });
  GPT_HIPCHK(hipStreamSynchronize(s->stream));
  if (rc != GPT_OK) return rc;
  double tot = 0.0;
  for (long long i = 0; i < nl; ++i) {
    float ms = 0.f;
    GPT_HIPCHK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
    tot += ms;
  }
  s->steps_done += cnt;
  if (avg_us) *avg_us = 1000.0 * tot / (double)cnt;
  return GPT_OK;
}

extern "C" int gpt_sgld_session_stamps(gpt_sgld_session* s, int64_t nsteps, int64_t* out) {
  if (!s || !out) { set_error("null argument"); return GPT_ERR_BAD_DIMS; }
  if (s->xmode) { set_error("stamps are not available on an X session"); return GPT_ERR_BAD_DIMS; }
  const long long cnt = std::min<long long>(nsteps, s->total_steps - s->steps_done);
  if (cnt <= 0) return GPT_OK;
  GPT_TRY(session_prime(s));
  // one slot row per workgroup of a step: D+1 per chain
  const size_t per = (size_t)(s->P.D + 1) * s->nchains * kStamps;
  DevMem buf;
  GPT_HIPCHK(buf.alloc<int64_t>(per * cnt));
  GPT_HIPCHK(buf.zero());
  StepParams P = s->P;
  GPT_TRY(session_launches(s, cnt, 1, [&](long long i, auto&& launch) {   // a launch per step
    P.stamps = buf.as<long long>() + per * i;
    return launch(P);
  }));
  GPT_HIPCHK(hipStreamSynchronize(s->stream));
  GPT_HIPCHK(buf.download(out, per * cnt));
  s->steps_done += cnt;
  return GPT_OK;
}

extern "C" int64_t gpt_sgld_timeline_slots(void) { return kTimeline; }

extern "C" int gpt_sgld_session_timeline(gpt_sgld_session* s, int64_t nsteps, int64_t* out,
                                         double* event_us) {
  if (!s || !out) { set_error("null argument"); return GPT_ERR_BAD_DIMS; }
  if (s->xmode) { set_error("the timeline is not available on an X session"); return GPT_ERR_BAD_DIMS; }
  if (s->engine != kEngineChain) { set_error("timeline: chain engine only"); return GPT_ERR_BAD_DIMS; }
  const long long left = s->total_steps - s->steps_done;
  const int span = session_span(s, s->steps_done, std::min<long long>(nsteps, left));
  if (nsteps < 1 || span != nsteps || nsteps > kTimelineSteps) {
    set_error("timeline: nsteps must be one launch (within the epoch and the run, <= 512)");
    return GPT_ERR_BAD_DIMS;
  }
  const size_t per = (size_t)kTimeline * s->nchains;
  DevMem buf;
  GPT_HIPCHK(buf.alloc<int64_t>(per));
  GPT_HIPCHK(hipMemsetAsync(buf.p, 0, buf.bytes, s->stream));
  StepParams P = s->P;
  P.tline = buf.as<long long>();
  ScopedEvents evs;
  GPT_HIPCHK(evs.create(2));
  GPT_TRY(session_launches(s, nsteps, kAnySpan, [&](long long, auto&& launch) {   // the one launch
    GPT_HIPCHK(hipEventRecord(evs.e[0], s->stream));
    GPT_TRY(launch(P));
    GPT_HIPCHK(hipEventRecord(evs.e[1], s->stream));
    return (int)GPT_OK;
  }));
  GPT_HIPCHK(hipStreamSynchronize(s->stream));
  float ms = 0.f;
  GPT_HIPCHK(hipEventElapsedTime(&ms, evs.e[0], evs.e[1]));
  if (event_us) *event_us = 1000.0 * ms;
  GPT_HIPCHK(buf.download(out, per));
  s->steps_done += nsteps;
  return GPT_OK;
}

extern "C" int gpt_sgld_session_info(gpt_sgld_session* s, int64_t* out) {
  if (!s || !out) { set_error("null argument"); return GPT_ERR_BAD_DIMS; }
  const StepParams& P = s->P;
  out[0] = s->engine;
  if (s->engine == kEngineChain) {
    out[1] = (int64_t)chain_lds_bytes(P.n, P.D, P.r, P.Q, P.m);
    out[2] = 64 * P.D;
    out[3] = s->nchains;
  } else if (s->engine == kEngineWave) {     // the dimension launch (the V-phase: one per chain)
    out[1] = (int64_t)wv_dim_lds_bytes(P.n, P.r, P.m);
    out[2] = 64;
    out[3] = (int64_t)P.D * s->nchains;
  } else {
    out[1] = (int64_t)step_layout(P.n, P.D, P.r, P.Q, P.m).bytes;
    out[2] = kNT;
    out[3] = (int64_t)(P.D + 1) * s->nchains;
  }
  return GPT_OK;
}

extern "C" int gpt_sgld_session_sync(gpt_sgld_session* s) {
  if (!s) return GPT_ERR_BAD_DIMS;
  GPT_HIPCHK(hipStreamSynchronize(s->stream));
  return GPT_OK;
}

extern "C" int64_t gpt_sgld_session_steps_done(gpt_sgld_session* s) { return s ? s->steps_done : -1; }

extern "C" int gpt_sgld_session_state(gpt_sgld_session* s, int32_t chain, double** w_dev,
                                      double** U_dev, double** w_store_dev, double** U_store_dev,
                                      int64_t* nstore) {
  if (!s || chain < 0 || chain >= s->nchains) { set_error("bad chain"); return GPT_ERR_BAD_DIMS; }
  const ChainDesc& C = s->chains_h[chain];
  // current w lives in the ping-pong slot of the next step
  if (w_dev) *w_dev = C.w + (size_t)(s->steps_done & 1) * s->P.Q;
  if (U_dev) *U_dev = C.U;
  if (w_store_dev) *w_store_dev = C.w_store;
  if (U_store_dev) *U_store_dev = C.U_store;
  if (nstore) *nstore = s->nstore;
  return GPT_OK;
}

extern "C" int gpt_sgld_session_gather_state(gpt_sgld_session* s, int32_t first, int32_t count,
                                             double* w_dev_out, double* U_dev_out) {
  if (!s || first < 0 || count < 0 || first + count > s->nchains || (count && (!w_dev_out || !U_dev_out))) {
    set_error("bad chain range"); return GPT_ERR_BAD_DIMS;
  }
  const size_t Q = (size_t)s->P.Q, nrD = (size_t)s->P.n * s->P.r * s->P.D;
  for (int32_t c = 0; c < count; ++c) {
    const ChainDesc& C = s->chains_h[first + c];
    GPT_HIPCHK(hipMemcpyAsync(w_dev_out + c * Q, C.w + (size_t)(s->steps_done & 1) * Q, 8 * Q,
                              hipMemcpyDeviceToDevice, s->stream));
    GPT_HIPCHK(hipMemcpyAsync(U_dev_out + c * nrD, C.U, 8 * nrD, hipMemcpyDeviceToDevice, s->stream));
  }
  return GPT_OK;
}

extern "C" int gpt_sgld_session_fetch(gpt_sgld_session* s, int32_t chain, double* w_store,
                                      double* U_store, double* diag, int32_t* status) {
  if (!s || chain < 0 || chain >= s->nchains) { set_error("bad chain"); return GPT_ERR_BAD_DIMS; }
  GPT_HIPCHK(hipStreamSynchronize(s->stream));
  const ChainDesc& C = s->chains_h[chain];
  int32_t st = 0;
  GPT_HIPCHK(hipMemcpy(&st, C.status, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (status) *status = st;
  const size_t nws = (size_t)s->P.Q * s->nstore, nus = (size_t)s->P.n * s->P.r * s->P.D * s->nstore;
  if (w_store) {
    if (!s->store) { set_error("session created without stores"); return GPT_ERR_BAD_DIMS; }
    if (st) std::memset(w_store, 0, 8 * nws);  // GPT_SGLD.jl:422-424
    else GPT_HIPCHK(hipMemcpy(w_store, C.w_store, 8 * nws, hipMemcpyDeviceToHost));
  }
  if (U_store) {
    if (!s->store) { set_error("session created without stores"); return GPT_ERR_BAD_DIMS; }
    if (st) std::memset(U_store, 0, 8 * nus);
    else GPT_HIPCHK(hipMemcpy(U_store, C.U_store, 8 * nus, hipMemcpyDeviceToHost));
  }
  if (diag) {
    if (!s->diag) { set_error("session created without diagnostics"); return GPT_ERR_BAD_DIMS; }
    GPT_HIPCHK(hipMemcpy(diag, C.diag, 8 * (size_t)(1 + s->P.D) * s->total_steps, hipMemcpyDeviceToHost));
  }
  return GPT_OK;
}

extern "C" void gpt_sgld_session_destroy(gpt_sgld_session* s) { delete s; }

// ====================================================================== test entries
// expm of `count` row-major nn × nn host matrices on the device, by the wave engine's
// register-blocked Padé (modes 0 and 4) or the grid engine's wave_expm (modes 1, 3 and 5); the
// (mode, nn) pairs are listed at wv_expm_check_kernel (wave.hip).
extern "C" int gpt_debug_expm(int32_t nn, int32_t count, int32_t mode, const double* A, double* E,
                              int32_t* bad) {
  if (count < 1 || !A || !E || !bad) { set_error("bad arguments"); return GPT_ERR_BAD_DIMS; }
  const size_t na = (size_t)nn * nn * count;
  DevMem dA, dE, dB;
  GPT_HIPCHK(dA.upload(A, na));
  GPT_HIPCHK(dE.alloc<double>(na));
  GPT_HIPCHK(dB.alloc<int32_t>(count));
  hipError_t e = launch_expm_check(nn, count, dA.as<double>(), dE.as<double>(), dB.as<int32_t>(),
                                   mode, nullptr);
  if (e == hipErrorInvalidValue) { set_error("(mode, nn) not instantiated"); return GPT_ERR_BAD_DIMS; }
  GPT_HIPCHK(e);
  GPT_HIPCHK(hipDeviceSynchronize());
  GPT_HIPCHK(dE.download(E, na));
  GPT_HIPCHK(dB.download(bad, count));
  return GPT_OK;
}

extern "C" int gpt_debug_gaussian_draw(int32_t p, const double* M, const double* x, uint64_t seed,
                                       uint32_t c1, uint32_t c2, uint32_t c3, double* out,
                                       int32_t* status) {
  if (p < 1 || !M || !x || !out || !status) { set_error("bad arguments"); return GPT_ERR_BAD_DIMS; }
  DevMem dM, dx, dz, dout, dst;
  GPT_HIPCHK(dM.upload(M, (size_t)p * p));
  GPT_HIPCHK(dx.upload(x, p));
  GPT_HIPCHK(dz.alloc<double>(p));
  GPT_HIPCHK(dout.alloc<double>(p));
  GPT_HIPCHK(dst.alloc<int32_t>(1));
  GPT_HIPCHK(dst.zero());
  GPT_HIPCHK(gaussian_draw_prec(dM.as<double>(), p, dx.as<double>(), seed, c1, c2, c3, dz.as<double>(),
                                dout.as<double>(), dst.as<int32_t>(), nullptr));
  GPT_HIPCHK(hipDeviceSynchronize());
  GPT_HIPCHK(dout.download(out, p));
  GPT_HIPCHK(dst.download(status, 1));
  return GPT_OK;
}

extern "C" int gpt_debug_expm_stamps(int32_t nn, int32_t count, const double* A, int64_t* stamps) {
  if (count < 1 || !A || !stamps) { set_error("bad arguments"); return GPT_ERR_BAD_DIMS; }
  const size_t na = (size_t)nn * nn * count;
  DevMem dA, dE, dB, dS;
  GPT_HIPCHK(dA.upload(A, na));
  GPT_HIPCHK(dE.alloc<double>(na));
  GPT_HIPCHK(dB.alloc<int32_t>(count));
  GPT_HIPCHK(dS.alloc<int64_t>(4 * (size_t)count));
  hipError_t e = launch_expm_check(nn, count, dA.as<double>(), dE.as<double>(), dB.as<int32_t>(), 2,
                                   nullptr, dS.as<long long>());
  if (e == hipErrorInvalidValue) { set_error("nn not instantiated"); return GPT_ERR_BAD_DIMS; }
  GPT_HIPCHK(e);
  GPT_HIPCHK(hipDeviceSynchronize());
  GPT_HIPCHK(dS.download(stamps, 4 * (size_t)count));
  return GPT_OK;
}
