// The frame the three resident hyper-parameter handles share (gpt_nlml in nlml.hip, gpt_egp in
// exactgp.hip, gpt_cjoint in api_cjoint.hip): the checks of the hyper-parameter vector
// and of a prediction's test arguments, the length scales and their gradient in the iso and ARD
// forms, the key of the resident factor, the phase marks of a timed evaluation, the scratch block
// that grows on demand, a prediction's test-side buffers and the one-shot form.  Host only.
#pragma once
#include <cmath>
#include <string>
#include "host_util.h"

namespace gpt {

// hyper = [length scales: D entries, or one (the iso form); `tail` further entries], every entry
// positive and finite.  `who` leads the message.
inline bool hyper_ok(const char* who, const double* hyper, int64_t Lh, int64_t D, int tail) {
  const std::string w(who);
  if (!hyper) { set_error(w + ": null hyperparams"); return false; }
  if (Lh != 1 + tail && Lh != D + tail) {
    set_error(w + ": hyperparams must have " + std::to_string(1 + tail) + " or D + " +
              std::to_string(tail) + " entries");
    return false;
  }
  for (int64_t k = 0; k < Lh; ++k)
    if (!(hyper[k] > 0.0) || !std::isfinite(hyper[k])) {
      set_error(w + ": hyperparams must be positive and finite");
      return false;
    }
  return true;
}

// ls[0..D) of a checked hyper: its own entry per dimension in the ARD form, the one entry in the
// iso form.  ls has room for kDMax.
inline void length_scales(const double* hyper, int64_t Lh, int D, int tail, double* ls) {
  for (int k = 0; k < D; ++k) ls[k] = hyper[Lh == D + tail ? k : 0];
}

// The leading entries of grad from the per-dimension gl: gl itself in the ARD form, its sum in
// dimension order in the iso form.
inline void fold_ls_grad(const double* gl, int D, int64_t Lh, int tail, double* grad) {
  if (Lh == D + tail) {
    for (int k = 0; k < D; ++k) grad[k] = gl[k];
  } else {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += gl[k];
    grad[0] = s;
  }
}

// The test arguments of a prediction.
inline bool test_args_ok(const char* who, const void* Xtest, int64_t Ntest, const void* ytest,
                         int64_t chunk, const void* fmu, const void* fs2, const void* lp) {
  const std::string w(who);
  if (!Xtest || !fmu || !fs2) { set_error(w + ": null test input or output"); return false; }
  if (lp && !ytest) { set_error(w + ": lp needs ytest"); return false; }
  if (Ntest < 1 || Ntest > (1LL << 31) - 1) { set_error(w + ": Ntest must be in 1..2^31-1"); return false; }
  if (chunk < 0) { set_error(w + ": chunk must be >= 0"); return false; }
  return true;
}

inline void nan_fill(double* p, int64_t n) {
  if (p) for (int64_t k = 0; k < n; ++k) p[k] = std::nan("");
}

// Which hyper-parameters the resident factor (or cache) of a handle stands for, compared by bits.
struct FactorKey {
  double last[kDMax + 2] = {0};
  int64_t last_Lh = 0;
  bool valid = false;
  bool matches(const double* hyper, int64_t Lh) const {
    return valid && last_Lh == Lh && std::memcmp(last, hyper, 8 * (size_t)Lh) == 0;
  }
  void set(const double* hyper, int64_t Lh) {           // Lh of a checked hyper: at most kDMax + 2
    std::memcpy(last, hyper, 8 * (size_t)Lh);
    last_Lh = Lh;
    valid = true;
  }
  void clear() { valid = false; }
};

// The phase marks of a timed evaluation: phases + 1 events, made by the handle's first timed call
// and kept with it.  begin() says whether this call is timed, mark() records the next event when
// it is, read() writes the times between the marks once the stream has drained.
struct PhaseMarks {
  ScopedEvents ev;
  int next = 0;
  bool on = false;
  hipError_t begin(bool timed, int phases) {
    on = timed;
    next = 0;
    return on && ev.e.empty() ? ev.create((size_t)phases + 1) : hipSuccess;
  }
  void mark(hipStream_t st) {
    if (on) (void)hipEventRecord(ev.e[next], st);
    ++next;
  }
  hipError_t read(double* phase_ms) const {
    for (size_t q = 0; on && q + 1 < ev.e.size(); ++q) {
      float ms = 0.f;
      const hipError_t r = hipEventElapsedTime(&ms, ev.e[q], ev.e[q + 1]);
      if (r != hipSuccess) return r;
      phase_ms[q] = ms;
    }
    return hipSuccess;
  }
};

// A device block of rows × cols doubles that grows when a call asks for more columns.
struct GrowBlock {
  double* p = nullptr;
  size_t cols = 0;
  DevMem mem;
  hipError_t reserve(size_t rows, size_t want) {
    if (cols >= want) return hipSuccess;
    p = nullptr;
    cols = 0;
    mem = DevMem();                      // the old block is freed before the larger one is taken
    const hipError_t e = mem.alloc<double>(rows * want);
    if (e == hipSuccess) { p = mem.as<double>(); cols = want; }
    return e;
  }
};

// The test-side device buffers of one prediction: mean and variance, and with lp the log density
// and the targets (which the caller copies in).
struct TestBuffers {
  DevSet mem;
  size_t count = 0;
  double *mu = nullptr, *v = nullptr, *lp = nullptr, *y = nullptr;
  hipError_t alloc(size_t Ntest, bool with_lp) {
    count = Ntest;
    hipError_t e = mem.alloc(&mu, Ntest);
    if (e == hipSuccess) e = mem.alloc(&v, Ntest);
    if (e == hipSuccess && with_lp) e = mem.alloc(&lp, Ntest);
    if (e == hipSuccess && with_lp) e = mem.alloc(&y, Ntest);
    return e;
  }
  // queued on st; the caller synchronises
  hipError_t download(double* fmu, double* fs2, double* lp_out, hipStream_t st) const {
    hipError_t e = hipMemcpyAsync(fmu, mu, 8 * count, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(fs2, v, 8 * count, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && lp_out)
      e = hipMemcpyAsync(lp_out, lp, 8 * count, hipMemcpyDeviceToHost, st);
    return e;
  }
};

// gpt_*_destroy: the device drains before the handle's memory goes.
template <class H> int destroy_handle(H* h) {
  if (h) {
    (void)hipDeviceSynchronize();
    delete h;
  }
  return GPT_OK;
}

// The one-shot form of a handle call: create(&h), body(h) on the fresh handle, destroy; the code
// of create when it fails, else that of body.
template <class H, class Create, class Body> int one_shot(Create&& create, Body&& body) {
  H* h = nullptr;
  GPT_TRY(create(&h));
  const int rc = body(h);
  destroy_handle(h);
  return rc;
}

}  // namespace gpt
