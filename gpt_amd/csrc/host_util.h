// Host-only helpers of the libgptsgld translation units: the HIP error check, the owners of device
// allocations and the argument idioms the C entries share.  No device code.
#pragma once
#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <utility>
#include <vector>
#include "gpt_internal.h"

namespace gpt {

#define GPT_HIPCHK(call)                               \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return hip_fail(_e, #call);  \
  } while (0)
// Return the first GPT_* code of a callee that is not GPT_OK.
#define GPT_TRY(call)                    \
  do {                                   \
    const int _rc = (call);              \
    if (_rc != GPT_OK) return _rc;       \
  } while (0)

// Owner of one device allocation.  Sizes are element counts of T: the byte count of a buffer is
// formed once, in alloc, and zero / download work from it.
struct DevMem {
  void* p = nullptr;
  size_t bytes = 0;
  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevMem& operator=(DevMem&& o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~DevMem() { if (p) (void)hipFree(p); }
  template <class T> hipError_t alloc(size_t count) {
    bytes = sizeof(T) * count;
    return hipMalloc(&p, bytes ? bytes : 16);
  }
  template <class T> hipError_t upload(const T* host, size_t count) {   // allocate and copy in
    const hipError_t e = alloc<T>(count);
    return e != hipSuccess ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
  }
  hipError_t zero() { return hipMemset(p, 0, bytes); }
  template <class T> hipError_t download(T* host, size_t count) const {
    if (sizeof(T) * count > bytes) return hipErrorInvalidValue;
    return hipMemcpy(host, p, sizeof(T) * count, hipMemcpyDeviceToHost);
  }
  template <class T> T* as() const { return (T*)p; }
};

// Owner of the many allocations of a handle object (freed together with it).
struct DevSet {
  std::vector<DevMem> mem;
  template <class T> hipError_t alloc(T** out, size_t count) {
    DevMem m;
    const hipError_t e = m.alloc<T>(count);
    if (e == hipSuccess) {
      *out = m.as<T>();
      mem.push_back(std::move(m));
    }
    return e;
  }
  template <class T> hipError_t upload(T** out, const T* host, size_t count) {
    const hipError_t e = alloc(out, count);
    return e != hipSuccess ? e : hipMemcpy(*out, host, sizeof(T) * count, hipMemcpyHostToDevice);
  }
};

// Carves typed arrays out of one device allocation.  Every array starts on a 256-byte boundary,
// the alignment of a hipMalloc of its own, so a kernel may assume of a carved pointer whatever it
// may of an allocated one.  The same take() calls run twice: without a base they count the bytes,
// with one they hand the arrays out and copy `host` in (the first failed copy is kept in err).
struct Carve {
  char* base = nullptr;
  size_t off = 0;
  hipError_t err = hipSuccess;
  template <class T> T* take(size_t count, const T* host = nullptr) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += (sizeof(T) * count + 255) / 256 * 256;
    if (p && host && err == hipSuccess) err = hipMemcpy(p, host, sizeof(T) * count, hipMemcpyHostToDevice);
    return p;
  }
};

// One device copy per distinct host array (the host pointers of sibling chains may repeat).
struct UploadCache {
  DevSet mem;
  std::unordered_map<const double*, const double*> dev_of;
};
inline hipError_t upload_once(UploadCache& uc, const double* h, size_t count, const double** out) {
  const auto it = uc.dev_of.find(h);
  if (it != uc.dev_of.end()) { *out = it->second; return hipSuccess; }
  double* d = nullptr;
  const hipError_t e = uc.mem.upload(&d, h, count);
  if (e == hipSuccess) *out = uc.dev_of[h] = d;
  return e;
}

// The 0-based table of the 1-based core index array I (Q × D); false with the error set when an
// entry is outside 1..r.
inline bool zero_based_I(const int32_t* I, int64_t Q, int64_t D, int64_t r,
                         std::vector<int32_t>& out) {
  out.resize((size_t)(Q * D));
  for (size_t x = 0; x < out.size(); ++x) {
    if (I[x] < 1 || I[x] > r) { set_error("I entries must be in 1..r"); return false; }
    out[x] = I[x] - 1;
  }
  return true;
}

// Events destroyed on every exit path.
struct ScopedEvents {
  std::vector<hipEvent_t> e;
  ~ScopedEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
  hipError_t create(size_t count) {
    e.assign(count, nullptr);
    for (auto& x : e) {
      const hipError_t r = hipEventCreate(&x);
      if (r != hipSuccess) return r;
    }
    return hipSuccess;
  }
};

// Device-event time in ms of the work put on st between construction and stop(), written to *ms
// when the timer goes out of scope (after the caller's synchronisation).
struct EventTimer {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t st;
  double* ms;
  EventTimer(double* ms_, hipStream_t st_) : st(st_), ms(ms_) {
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
    (void)hipEventRecord(a, st);
  }
  EventTimer(const EventTimer&) = delete;
  EventTimer& operator=(const EventTimer&) = delete;
  void stop() { if (b) (void)hipEventRecord(b, st); }
  ~EventTimer() {
    float t = 0.0f;
    if (a && b && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&t, a, b) == hipSuccess)
      *ms = t;
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// ---- sibling full-theta chains (gpt_gpnt_sgld_chains*, gpt_gpnt_sgld_class_chains) -------------
// The bounds the two entries share; each adds its own bound on m and its own message.
inline bool theta_chain_dims_ok(int64_t n, int64_t N, int64_t m, int64_t burnin, int64_t maxepoch,
                                int32_t nchains, int64_t store_every) {
  return n >= 1 && N >= 1 && m >= 1 && burnin >= 0 && maxepoch >= 0 && nchains >= 1 &&
         store_every >= 1 && n <= (1 << 20) && N <= (1LL << 31) - 1 && nchains <= 65535 &&
         store_every <= (1 << 30) && burnin + maxepoch <= (1 << 24);
}
// A run's step counts: nb batches per epoch, total steps, of which kept are stored.
struct ThetaRun {
  int epochs = 0;
  long long nb = 0, total = 0, kept = 0;
  ThetaRun() = default;
  ThetaRun(int64_t N, int64_t m, int64_t burnin, int64_t maxepoch, int64_t store_every)
      : epochs((int)(burnin + maxepoch)), nb((N + m - 1) / m), total(epochs * nb),
        kept(total / store_every) {}
};
// The device state of nchains sibling chains whose theta has len = n·C doubles, and the launch
// loop over it.  An entry builds its descriptors on chain(k) and gives run() its kernel launch.
struct ThetaChainSet {
  DevMem ord, theta, store, status;
  std::vector<size_t> ord_at;     // chain k's epoch orders start at ord + ord_at[k]
  const uint64_t* seeds;
  const double* eps_theta;
  size_t nchains, len, kept;
  // Epoch orders, one set per distinct seed; theta0[:, c] of chain k =
  // sigma_theta[k·sigma_stride]·normals(n, seeds[k], 0, THETA_INIT, c); a zeroed store and status.
  int init(const uint64_t* seeds_, const double* eps_theta_, int nchains_, int64_t n, int C,
           int64_t N, const ThetaRun& R, const double* sigma_theta, int sigma_stride) {
    seeds = seeds_; eps_theta = eps_theta_; nchains = nchains_; len = (size_t)n * C; kept = R.kept;
    std::unordered_map<uint64_t, size_t> ord_of;
    const size_t per = (size_t)R.epochs * N;
    for (size_t k = 0; k < nchains; ++k)
      ord_at.push_back(per * ord_of.emplace(seeds[k], ord_of.size()).first->second);
    std::vector<int32_t> o(per * ord_of.size());
    for (const auto& kv : ord_of) host_epoch_orders((int)N, kv.first, R.epochs, o.data() + per * kv.second);
    std::vector<double> th0(len * nchains);
    for (size_t k = 0; k < nchains; ++k)
      for (int c = 0; c < C; ++c)
        for (int64_t j = 0; j < n; ++j)
          th0[len * k + (size_t)n * c + j] = sigma_theta[k * sigma_stride] *
              host_normal(seeds[k], (uint32_t)j, 0, kThetaInit, (uint32_t)c);
    GPT_HIPCHK(ord.upload(o.data(), o.size()));
    GPT_HIPCHK(theta.upload(th0.data(), th0.size()));
    GPT_HIPCHK(store.alloc<double>(len * kept * nchains));
    GPT_HIPCHK(status.alloc<int32_t>(nchains));
    GPT_HIPCHK(status.zero());
    GPT_HIPCHK(store.zero());
    return GPT_OK;
  }
  ThetaChain chain(int k) const {
    return {ord.as<int32_t>() + ord_at[k], theta.as<double>() + len * k,
            store.as<double>() + len * kept * k, status.as<int32_t>() + k, seeds[k], eps_theta[k]};
  }
  // launch(t0, nsteps) for every epoch in chunks of at most 4096 steps, timed into *ms by device
  // events around the launches; then the status and the store come back, the store of a chain
  // that met a NaN zero-filled (GPT_SGLD.jl:840-843 / :894-897).
  template <class Launch>
  int run(const ThetaRun& R, double* ms, const char* what, Launch&& launch, double* theta_store,
          int32_t* status_out) const {
    const int chunk = (int)std::min<long long>(R.nb, 4096);    // steps per launch, within an epoch
    {
      EventTimer tm(ms, nullptr);
      for (int e = 0; e < R.epochs; ++e)
        for (long long b0 = 0; b0 < R.nb; b0 += chunk) {
          const hipError_t er = launch(e * R.nb + b0, (int)std::min<long long>(chunk, R.nb - b0));
          if (er != hipSuccess) return hip_fail(er, what);
        }
      tm.stop();
      GPT_HIPCHK(status.download(status_out, nchains));
    }
    GPT_HIPCHK(store.download(theta_store, len * kept * nchains));
    for (size_t k = 0; k < nchains; ++k)
      if (status_out[k]) std::memset(theta_store + len * kept * k, 0, 8 * len * kept);
    return GPT_OK;
  }
};

}  // namespace gpt
