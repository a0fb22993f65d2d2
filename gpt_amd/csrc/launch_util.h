// Host-side launch plumbing shared by every templated kernel family: the table of instantiated
// template values, one run-time -> compile-time dispatcher over such a table, and the launch
// helpers (one of which owns the dynamic-LDS opt-in).  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>
#include <type_traits>

namespace gpt {

// ---- the instantiation table ------------------------------------------------------------------
template <int... Vs> struct IntList {};
template <int V> using Int = std::integral_constant<int, V>;

// Tensor ranks r every grid / prediction / TGP / CF kernel is instantiated for.  Adding a rank is
// one entry here (plus whatever the kernels themselves need at that rank).
using Ranks = IntList<1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 16, 20>;
// Wave engine (wave.hip): the ranks past the chain engine, and the dimensions per wave J
using WaveRanks = IntList<6, 8, 10, 12, 15, 16, 20>;
using WaveJs = IntList<1, 2, 3, 4>;
// Chain engine (chain.hip): rank R, dimensions per wave J, U-phase waves WV (wide | 4)
using ChainRanks = IntList<1, 2, 3, 4, 5>;
using ChainJs = IntList<1, 2, 4, 8>;
using ChainWVs = IntList<8, 4>;

template <int... Vs> constexpr bool contains(IntList<Vs...>, int v) { return ((v == Vs) || ...); }

inline bool rank_supported(int r) { return contains(Ranks{}, r); }

// "1-6,8,10,12,15,16,20": the list, runs of three or more consecutive values as a range
template <int... Vs> std::string list_text(IntList<Vs...>) {
  const int v[] = {Vs...}, n = (int)sizeof...(Vs);
  std::string s;
  for (int i = 0, j; i < n; i = j + 1) {
    for (j = i; j + 1 < n && v[j + 1] == v[j] + 1;) ++j;
    if (j == i + 1) j = i;
    if (i) s += ',';
    s += std::to_string(v[i]);
    if (j > i) s += '-' + std::to_string(v[j]);
  }
  return s;
}
inline std::string ranks_text() { return list_text(Ranks{}); }

// ---- the dispatcher ---------------------------------------------------------------------------
// f(Int<V>{}) for the V of the list equal to v, `none` when v is not in the list.  Choices over
// several template parameters nest it.
template <int... Vs, class T, class F> T with_value_or(IntList<Vs...>, int v, T none, F&& f) {
  (void)((v == Vs && ((none = f(Int<Vs>{})), true)) || ...);
  return none;
}
// The launchers' form: f launches and returns its error; a v outside the list is an invalid value.
template <int... Vs, class F> hipError_t with_value(IntList<Vs...> l, int v, F&& f) {
  return with_value_or(l, v, hipErrorInvalidValue, f);
}
template <class F> hipError_t with_rank(int r, F&& f) { return with_value(Ranks{}, r, f); }

constexpr int kMaxLds = 160 * 1024;   // the LDS of a CDNA4 workgroup

// ---- launches ---------------------------------------------------------------------------------
// Raise a kernel's dynamic-LDS limit once per device.  Thread-safe: host threads (one per GPU, or
// several sessions) may race to set the same attribute, which is idempotent; the latch only
// skips the call once a device has it.
inline hipError_t set_max_lds_once(const void* fn, int bytes, std::atomic<uint64_t>& latch) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (latch.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) latch.fetch_or(bit, std::memory_order_acq_rel);
  return e;
}

// The plain launch.  It raises no limit: for kernels that never need more than the default 64 KiB
// of LDS, and for the grid kernels, whose limit set_lds_limits() raised when the session was made.
template <auto Kernel, class... A>
hipError_t launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, A... a) {
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, a...);
  return hipGetLastError();
}

// Kernels that may need more: the first launch on a device opts Kernel into max_bytes of dynamic
// LDS.  One latch per kernel, whatever the types of the arguments at the call.
template <auto Kernel> std::atomic<uint64_t>& lds_latch() {
  static std::atomic<uint64_t> latch{0};
  return latch;
}
template <auto Kernel, class... A>
hipError_t launch_big_lds(int max_bytes, dim3 grid, dim3 block, size_t lds, hipStream_t st,
                          A... a) {
  const hipError_t e = set_max_lds_once((const void*)Kernel, max_bytes, lds_latch<Kernel>());
  if (e != hipSuccess) return e;
  return launch<Kernel>(grid, block, lds, st, a...);
}

// Kernels that rarely do: the opt-in only when this launch is past the default 64 KiB
template <auto Kernel, class... A>
hipError_t launch_lds_over_64k(int max_bytes, dim3 grid, dim3 block, size_t lds, hipStream_t st,
                               A... a) {
  return lds > 64 * 1024 ? launch_big_lds<Kernel>(max_bytes, grid, block, lds, st, a...)
                         : launch<Kernel>(grid, block, lds, st, a...);
}

}  // namespace gpt
