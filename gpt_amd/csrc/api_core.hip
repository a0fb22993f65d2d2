// Host side of libgptsgld.so: the C ABI of include/gptsgld.h (api_*.hip, one file per object).
//
// Replaces the Julia module API of GPT_SGLD.jl (feature :71, featureNotensor :109, samplenz :181,
// GPTregression :345, pred :233, GPNT_SGLD :809) and GPT_SGLD_p.jl (GPT_SGLDERM :146, RMSE :124).
// All arithmetic of the sampler runs in the HIP kernels; the host only validates arguments,
// draws the one-time initial state and the epoch permutations from the Philox contract (the
// reference does the same draws on the CPU, GPT_SGLD.jl:357-373), moves buffers and launches.
//
// This file: the error state, the host Philox draws and the entries that need no session.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_util.h"

namespace gpt {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return GPT_ERR_HIP;
}

// ------------------------------------------------------------------ host Philox consumers
double host_normal(uint64_t seed, uint32_t e, uint32_t c1, uint32_t c2, uint32_t c3) {
  const U4 x = philox4x32(e >> 1, c1, c2, c3, seed);
  const double u1 = u53(x.x, x.y), u2 = u53(x.z, x.w);
  const double rad = std::sqrt(-2.0 * std::log(u1));
  const double th = 6.283185307179586 * u2;
  return (e & 1u) ? rad * std::sin(th) : rad * std::cos(th);
}

// Cyclic Jacobi eigendecomposition of a symmetric r×r matrix (row-major, destroyed).
static void jacobi_eig(int r, std::vector<double>& A, std::vector<double>& V,
                       std::vector<double>& ev) {
  V.assign((size_t)r * r, 0.0);
  for (int i = 0; i < r; ++i) V[i * r + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < r; ++j) {
        tot += A[i * r + j] * A[i * r + j];
        if (i != j) off += A[i * r + j] * A[i * r + j];
      }
    if (off <= 1e-32 * tot) break;
    for (int p = 0; p < r; ++p)
      for (int q = p + 1; q < r; ++q) {
        const double apq = A[p * r + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * r + q] - A[p * r + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < r; ++k) {  // A = Jᵀ A J
          const double akp = A[k * r + p], akq = A[k * r + q];
          A[k * r + p] = c * akp - s * akq;
          A[k * r + q] = s * akp + c * akq;
        }
        for (int k = 0; k < r; ++k) {
          const double apk = A[p * r + k], aqk = A[q * r + k];
          A[p * r + k] = c * apk - s * aqk;
          A[q * r + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < r; ++k) {
          const double vkp = V[k * r + p], vkq = V[k * r + q];
          V[k * r + p] = c * vkp - s * vkq;
          V[k * r + q] = s * vkp + c * vkq;
        }
      }
  }
  ev.resize(r);
  for (int i = 0; i < r; ++i) ev[i] = A[i * r + i];
}

// GPT_SGLD.jl:357-369: w = σ_w·randn(Q); U_k = Zᵀ(ZZᵀ)^(-1/2), Z = randn(r,n)  (or randn/√n).
// Uniform draw on the Stiefel manifold from Z (r × n, element a + r·j): Uk (n × r, column-major)
// = Zᵀ(ZZᵀ)^(-1/2), the polar factor (transpose(sqrtm(Z*Z') \\ Z), GPT_SGLD.jl:365-366).
void host_stiefel_polar(const double* Z, int r, int n, double* Uk) {
  std::vector<double> G((size_t)r * r, 0.0), Vv, ev;
  for (int a = 0; a < r; ++a)
    for (int c = 0; c < r; ++c) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += Z[a + (size_t)r * j] * Z[c + (size_t)r * j];
      G[a * r + c] = s;
    }
  jacobi_eig(r, G, Vv, ev);
  std::vector<double> S((size_t)r * r, 0.0);  // (ZZᵀ)^(-1/2)
  for (int a = 0; a < r; ++a)
    for (int c = 0; c < r; ++c) {
      double s = 0.0;
      for (int z = 0; z < r; ++z) s += Vv[a * r + z] * Vv[c * r + z] / std::sqrt(ev[z]);
      S[a * r + c] = s;
    }
  for (int j = 0; j < n; ++j)
    for (int c = 0; c < r; ++c) {
      double s = 0.0;
      for (int a = 0; a < r; ++a) s += Z[a + (size_t)r * j] * S[a * r + c];
      Uk[j + (size_t)n * c] = s;
    }
}

// Class cls of GPTclassification (GPT_SGLD.jl:463-477) draws w on (W_INIT, cls) and U_k on
// (U_INIT, k + D·cls), and its non-Stiefel U is randn unscaled (cls_init).
void host_init_state(int n, int r, int D, int Q, uint64_t seed, bool stiefel, double sigma_w,
                     double* w, double* U, int cls, bool cls_init) {
  for (int q = 0; q < Q; ++q) w[q] = sigma_w * host_normal(seed, q, 0, kWInit, (uint32_t)cls);
  std::vector<double> Z((size_t)r * n);
  for (int k = 0; k < D; ++k) {
    for (int e = 0; e < r * n; ++e) Z[e] = host_normal(seed, e, 0, kUInit, (uint32_t)(k + D * cls));  // Z[a + r*j]
    double* Uk = U + (size_t)n * r * k;
    if (!stiefel) {
      for (int j = 0; j < n; ++j)
        for (int a = 0; a < r; ++a) Uk[j + (size_t)n * a] = cls_init ? Z[a + (size_t)r * j] : Z[a + (size_t)r * j] / std::sqrt((double)n);
      continue;
    }
    host_stiefel_polar(Z.data(), r, n, Uk);
  }
}

// Cumulative epoch orders on the host (GPNT_SGLD only; sessions build them on the device, order.hip):
// phi=phi[:,:,perm] every epoch composes the permutations (GPT_SGLD.jl:373-374);
// order_e = order_{e-1}[perm_e], perm_e Fisher–Yates on the PERM stream.
void host_epoch_orders(int N, uint64_t seed, int epochs, int32_t* out) {
  std::vector<int32_t> cur(N), p(N);
  for (int i = 0; i < N; ++i) cur[i] = i;
  for (int e = 0; e < epochs; ++e) {
    for (int i = 0; i < N; ++i) p[i] = i;
    for (int i = N - 1; i >= 1; --i) {
      const uint32_t x = philox4x32((uint32_t)i, (uint32_t)e, kPerm, 0, seed).x;
      const int j = (int)(((uint64_t)x * (uint64_t)(i + 1)) >> 32);
      std::swap(p[i], p[j]);
    }
    int32_t* o = out + (size_t)e * N;
    for (int i = 0; i < N; ++i) o[i] = cur[p[i]];
    std::memcpy(cur.data(), o, sizeof(int32_t) * N);
  }
}

bool valid_cfg(const gpt_sgld_config* c) {
  if (!c) { set_error("null config"); return false; }
  if (c->n < 1 || c->D < 1 || c->N < 1 || c->r < 1 || c->Q < 1 || c->m < 1) {
    set_error("dimensions must be positive"); return false;
  }
  if (c->D > kDMax) { set_error("D > 16 is not supported by the kernels"); return false; }
  if (!rank_supported((int)c->r)) {
    set_error("rank r not instantiated (supported: " + ranks_text() + ")"); return false;
  }
  if (c->n > (1 << 20) || c->N > (1LL << 31) - 1 || c->Q > (1 << 20)) {
    set_error("dimension too large"); return false;
  }
  double rD = std::pow((double)c->r, (double)c->D);
  if ((double)c->Q > rD) { set_error("Q must be <= r^D"); return false; }
  if (c->store_every < 1) { set_error("store_every must be >= 1"); return false; }
  if (!(c->signal_var > 0) || !(c->sigma_w > 0)) { set_error("variances must be > 0"); return false; }
  const StepLayout L = step_layout((int)c->n, (int)c->D, (int)c->r, (int)c->Q, (int)c->m);
  const bool chain_ok = chain_supported((int)c->n, (int)c->D, (int)c->r, (int)c->Q, (int)c->m,
                                        c->langevin != 0, c->stiefel != 0);
  const bool wave_ok = wave_supported((int)c->n, (int)c->D, (int)c->r, (int)c->Q, (int)c->m,
                                       c->langevin != 0, c->stiefel != 0);
  if (L.bytes > kMaxLds && !chain_ok && !wave_ok) {
    set_error("working set exceeds 160 KiB LDS (n*r, Q*D or m too large)"); return false;
  }
  return true;
}

}  // namespace gpt

using namespace gpt;

extern "C" const char* gpt_last_error(void) { return g_err.c_str(); }

extern "C" int64_t gpt_sgld_lds_bytes(int64_t n, int64_t D, int64_t r, int64_t Q, int64_t m) {
  return (int64_t)step_layout((int)n, (int)D, (int)r, (int)Q, (int)m).bytes;
}

extern "C" int gpt_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

extern "C" int gpt_sgld_init(const gpt_sgld_config* cfg, double* w_out, double* U_out) {
  if (!valid_cfg(cfg)) return GPT_ERR_BAD_DIMS;
  host_init_state((int)cfg->n, (int)cfg->r, (int)cfg->D, (int)cfg->Q, cfg->seed, cfg->stiefel != 0,
                  cfg->sigma_w, w_out, U_out);
  return GPT_OK;
}

extern "C" int gpt_samplenz(int64_t r, int64_t D, int64_t Q, uint64_t seed, int32_t* I_out) {
  if (r < 1 || D < 1 || Q < 1 || !I_out) { set_error("bad samplenz arguments"); return GPT_ERR_BAD_DIMS; }
  unsigned __int128 M = 1;
  for (int k = 0; k < D; ++k) {
    M *= (unsigned __int128)r;
    if (M > ((unsigned __int128)1 << 62)) { set_error("r^D too large"); return GPT_ERR_BAD_DIMS; }
  }
  if ((unsigned __int128)Q > M) { set_error("Q must be <= r^D"); return GPT_ERR_BAD_DIMS; }
  const uint64_t MM = (uint64_t)M;
  std::unordered_map<uint64_t, uint64_t> sw;
  auto get = [&sw](uint64_t x) { auto it = sw.find(x); return it == sw.end() ? x : it->second; };
  for (int64_t i = 0; i < Q; ++i) {
    const U4 x = philox4x32((uint32_t)i, 0, kSampleNZ, 0, seed);
    const uint64_t u = ((uint64_t)x.x << 32) | x.y;
    const uint64_t j = (uint64_t)i + (uint64_t)(((unsigned __int128)u * (MM - (uint64_t)i)) >> 64);
    const uint64_t vi = get(i), vj = get(j);
    sw[i] = vj;
    sw[j] = vi;
    uint64_t v = vj;  // L[i]; I[i,:] = digits(L, r, D) + 1
    for (int64_t k = 0; k < D; ++k) {
      I_out[i + Q * k] = (int32_t)(v % (uint64_t)r) + 1;
      v /= (uint64_t)r;
    }
  }
  return GPT_OK;
}

extern "C" int gpt_feature_inputs(int64_t n, int64_t D, uint64_t seed, double* Z_out, double* b_out) {
  if (n < 1 || D < 1) { set_error("bad dims"); return GPT_ERR_BAD_DIMS; }
  for (int64_t e = 0; e < n * D; ++e) {
    if (Z_out) Z_out[e] = host_normal(seed, (uint32_t)e, 0, kFeatZ, 0);
    if (b_out) {
      const U4 x = philox4x32((uint32_t)e, 0, kFeatB, 0, seed);
      b_out[e] = 2.0 * 3.141592653589793 * u53(x.x, x.y);
    }
  }
  return GPT_OK;
}

// Generation-A feature inputs (GPT_SGLD_p.jl:40-54): Z = randn(n,D) (the Gen-C Z stream) and
// b = randn(n,D) on the FEAT_B stream with c3 = 1 (Gen C draws b = 2π·rand on c3 = 0).
extern "C" int gpt_feature_inputs_a(int64_t n, int64_t D, uint64_t seed, double* Z_out, double* b_out) {
  if (n < 1 || D < 1) { set_error("bad dims"); return GPT_ERR_BAD_DIMS; }
  for (int64_t e = 0; e < n * D; ++e) {
    if (Z_out) Z_out[e] = host_normal(seed, (uint32_t)e, 0, kFeatZ, 0);
    if (b_out) b_out[e] = host_normal(seed, (uint32_t)e, 0, kFeatB, 1);
  }
  return GPT_OK;
}

// randperm(N) + phi = phi[:,:,perm] (GPT_SGLD.jl:373-374) for `epochs` epochs, built on the device
// by the sampler's own kernel (order.hip).  out: (N, epochs) column-major, 0-based rows.
extern "C" int gpt_epoch_orders(int64_t N, uint64_t seed, int64_t epochs, int32_t* out) {
  if (N < 1 || N > (1LL << 31) - 1 || epochs < 0 || epochs > (1 << 20) || (epochs && !out)) {
    set_error("bad epoch-order arguments"); return GPT_ERR_BAD_DIMS;
  }
  DevMem ring, cd, ws;
  GPT_HIPCHK(ring.alloc<int32_t>(2 * (size_t)N));
  ChainDesc C{};
  C.order = ring.as<int32_t>();
  C.seed = seed;
  GPT_HIPCHK(cd.upload(&C, 1));
  if (const size_t wsi = epoch_order_ws_ints((int)N, 1)) GPT_HIPCHK(ws.alloc<int32_t>(wsi));
  for (int64_t e = 0; e < epochs; ++e) {
    GPT_HIPCHK(launch_epoch_order(cd.as<ChainDesc>(), 1, (int)N, 1, 0, nullptr, 0, (int)e,
                                  ws.as<int32_t>(), nullptr));
    GPT_HIPCHK(hipMemcpy(out + (size_t)e * N, ring.as<int32_t>() + (size_t)(e & 1) * N,
                         4 * (size_t)N, hipMemcpyDeviceToHost));
  }
  return GPT_OK;
}
