// A pixel criterion over a RAGGED SET of tensor pairs in one launch each way: the VGG perceptual loss outside its network
// (GAN-Based-SR/basicsr/losses/basic_loss.py:212-251, `percep_loss += criterion(x_features[k], gt_features[k]) *
// layer_weights[k]` in a Python loop over the tapped layers, and the same over their Gram matrices; train_BSGRAN/
// models/loss.py:114-130).  The pairs differ in size by three orders of magnitude, so the launch is cut into chunks of
// one tensor each, as ssg_multi.hip cuts a parameter set, and summed as ssg_stream.hpp sums one tensor.
//
// Contract (this file is compiled with -ffp-contract=off; every fp32 operation is rounded on its own).  For the pairs
// (x_k, g_k, n_k, w_k), k < K, fp32, and d = x_k[i] - g_k[i] (one subtraction):
//   SSG_PIX_L1, _MSE, _CHARBONNIER   l and l' of ssg_stream.hpp's crit / dcrit: the functions of ssg_pixel_sums / _grad
//   SSG_PIX_FRO                      l = d d (crit of SSG_PIX_MSE), l' = d; the pair's term is sqrt(S_k)
//   sums     S_k = sum_i l(d_i): every fp32 l is widened and added in fp64.  A chunk is mcrit_chunk() elements of ONE
//            tensor (its last chunk what is left).  A workgroup of 256 threads takes chunk c = blockIdx.x, then c +
//            gridDim.x, ... (at most mcrit_grid_cap() workgroups); a thread adds its elements in index order, the
//            workgroup folds as ssg_stream.hpp folds, and ONE fp64 partial per chunk goes to the workspace.  A second
//            launch of one workgroup folds every tensor's partials in chunk order (thread i takes i, i + 256, ...,
//            then an LDS tree), writes S_k and adds w_k S_k (FRO: w_k sqrt(S_k)) in pair order into the total at [K].
//            No atomics.  S_k depends on x_k, g_k, n_k and their alignment alone: whichever other pairs are in the call,
//            it is the same bits.
//   grads    grad_k[i] = (float)(c_k (double)l'(d_i)), c_k = coef[0] w_k in fp64; FRO: c_k = coef[0] w_k / sqrt(S_k), and
//            0 where S_k = 0 (torch's norm backward).  coef and S are read on the device.  A pair without a gradient
//            pointer has no chunk in the launch.
// Chunks, their schedule and their walk are ssg_chunked.hpp's: the walked tensor is x; g and grad are accessed 16 bytes
// wide where they share x's alignment, element by element where they do not.
// The pair records travel BY VALUE in the kernel's arguments, MAX_PAIRS to a launch (feature maps move from step to step:
// a resident table would have to be uploaded every time); a larger set takes further launches into disjoint partial ranges.
// LDS holds the folds only; no scratch.  The launchers trust their arguments: the entry points below refuse bad ones.
#include "ssg_chunked.hpp"

namespace ssg {
namespace mcrit {

using namespace chunked;

constexpr int CHUNK = 8192;        // elements per chunk: eight float4 trips of a workgroup; the fastest of 4,096, 8,192
                                   // and 16,384 (profiles/perceptual_time.txt)
constexpr int GRID_CAP = MAX_WG;   // the scaffold's: four workgroups per CU
constexpr int MAX_PAIRS = 16;      // records per launch: 16 x 56 bytes of kernel arguments

SSG_TUNING tuning = {CHUNK, GRID_CAP};   // ssg_prof_mcrit_tuning: the A/B of profiles/perceptual_time.txt

struct Pair {
  const float *x, *g;
  float *grad;
  size_t n;
  double w;
  unsigned first;    // the pair's first chunk, counted inside its launch
  unsigned chunks;
  int index;         // k: where S_k lies
};

struct Set {
  Pair p[MAX_PAIRS];
  int K;
  unsigned n_chunks, chunk;
};

// the pair of a chunk, by compare and select over all the records (they are kernel arguments: no table in memory)
__device__ __forceinline__ Pair pair_of_chunk(const Set &s, unsigned c) {
  Pair cur = s.p[0];
#pragma unroll
  for (int k = 1; k < MAX_PAIRS; ++k) {
    if (k < s.K && c >= s.p[k].first) cur = s.p[k];
  }
  return cur;
}

// the element function of a kind: FRO sums squares and differentiates to d (its 1 / sqrt(S) is in the coefficient)
template <int KIND>
__device__ __forceinline__ float value(float d, float eps) {
  return crit<KIND == SSG_PIX_FRO ? SSG_PIX_MSE : KIND>(d, eps);
}

template <int KIND>
__device__ __forceinline__ float slope(float d, float eps) {
  if (KIND == SSG_PIX_FRO) return d;
  return dcrit<KIND == SSG_PIX_FRO ? SSG_PIX_MSE : KIND>(d, eps);
}

template <int KIND>
__global__ __launch_bounds__(NT) void mcrit_sums_kernel(const Set s, float eps, double *part) {
  for (unsigned c = blockIdx.x; c < s.n_chunks; c += gridDim.x) {
    const Pair p = pair_of_chunk(s, c);
    const Span sp = span_of(p.n, c - p.first, s.chunk);
    const float *x = p.x + sp.off, *g = p.g + sp.off;
    const bool gv = wide(g, head_of(x, sp.len));
    double L = 0.0;
    walk_chunk(
        x, sp.len, [&](unsigned e) { L += (double)value<KIND>(x[e] - g[e], eps); },
        [&](unsigned e) {
          float a[4], b[4];
          load4(x + e, true, a);
          load4(g + e, gv, b);
          for (int k = 0; k < 4; ++k) L += (double)value<KIND>(a[k] - b[k], eps);
        });
    workgroup_fold<1>({L}, part + c);
    __syncthreads();   // (the fold's LDS words are written again in the next trip)
  }
}

// one workgroup: S_k of every pair of the launch from its chunk partials, and the weighted total carried on from the
// launches before it (carry) at sums[total_at]
__global__ __launch_bounds__(NT) void mcrit_fold_kernel(const Set s, int fro, int carry, const double *part, double *sums,
                                                        int total_at) {
  __shared__ double sh[NT];
  const unsigned t = threadIdx.x;
  double total = carry ? sums[total_at] : 0.0;
  for (int k = 0; k < s.K; ++k) {
    const Pair &p = s.p[k];   // (read where it lies in the kernel's arguments: no copy of the records is made)
    double a = 0.0;
    for (unsigned i = t; i < p.chunks; i += NT) a += part[p.first + i];
    sh[t] = a;
    __syncthreads();
    for (unsigned o = NT / 2; o > 0; o >>= 1) {
      if (t < o) sh[t] += sh[t + o];
      __syncthreads();
    }
    if (t == 0) {
      const double S = sh[0];
      sums[p.index] = S;
      const double term = p.w * (fro ? sqrt(S) : S);
      total += term;
    }
    __syncthreads();
  }
  if (t == 0) sums[total_at] = total;
}

template <int KIND>
__global__ __launch_bounds__(NT) void mcrit_grad_kernel(const Set s, float eps, const double *coef, const double *S) {
  const double c0 = coef[0];
  for (unsigned c = blockIdx.x; c < s.n_chunks; c += gridDim.x) {
    const Pair p = pair_of_chunk(s, c);
    double ck = c0 * p.w;
    if (KIND == SSG_PIX_FRO) {
      const double Sk = S[p.index];
      ck = Sk == 0.0 ? 0.0 : ck / sqrt(Sk);
    }
    const Span sp = span_of(p.n, c - p.first, s.chunk);
    const float *x = p.x + sp.off, *g = p.g + sp.off;
    float *out = p.grad + sp.off;
    const size_t head = head_of(x, sp.len);
    const bool gv = wide(g, head), ov = wide(out, head);
    walk_chunk(
        x, sp.len, [&](unsigned e) { out[e] = (float)(ck * (double)slope<KIND>(x[e] - g[e], eps)); },
        [&](unsigned e) {
          float a[4], b[4], r[4];
          load4(x + e, true, a);
          load4(g + e, gv, b);
          for (int k = 0; k < 4; ++k) r[k] = (float)(ck * (double)slope<KIND>(a[k] - b[k], eps));
          store4(out + e, ov, r);
        });
  }
}

// ---- host ----
// Cuts the pairs k with keep(k) into launches of at most MAX_PAIRS records and calls go(set, first chunk of the launch
// among the kept pairs' chunks, whether it is the first launch); stops at the first status that is not 0.
template <class Keep, class Go>
inline int for_each_launch(size_t K, const size_t *x, const size_t *g, const size_t *grad, const size_t *counts,
                           const double *w, Keep keep, Go go) {
  Set s;
  s.K = 0, s.n_chunks = 0, s.chunk = (unsigned)tuning.chunk;
  size_t base = 0;
  bool first = true;
  for (size_t k = 0; k <= K; ++k) {
    if (k < K && keep(k)) {
      Pair &p = s.p[s.K++];
      p.x = (const float *)x[k], p.g = (const float *)g[k], p.grad = grad ? (float *)grad[k] : nullptr;
      p.n = counts[k], p.w = w[k], p.first = s.n_chunks, p.chunks = (unsigned)chunks_of(counts[k], s.chunk);
      p.index = (int)k;
      s.n_chunks += p.chunks;
    }
    if (s.K == MAX_PAIRS || (k == K && s.K > 0)) {
      for (int i = s.K; i < MAX_PAIRS; ++i) s.p[i] = s.p[0];   // (never selected: defined bytes for the launch)
      if (const int rc = go(s, base, first)) return rc;
      base += s.n_chunks, first = false;
      s.K = 0, s.n_chunks = 0;
    }
  }
  return 0;
}

// what the two entry points check of the pairs; `grad` may be null (the sums call) and may hold null addresses
static int check_pairs(size_t K, const size_t *x, const size_t *g, const size_t *grad, const size_t *counts,
                       const double *w, int kind, float eps, size_t *total) {
  if (K < 1 || K > (size_t)INT_MAX || !x || !g || !counts || !w) return SSG_E_BADARG;
  if (kind < SSG_PIX_L1 || kind > SSG_PIX_FRO) return SSG_E_BADARG;
  if (!(eps >= 0.f && eps <= 3.402823466e38f)) return SSG_E_BADARG;   // (a NaN fails both comparisons)
  for (size_t k = 0; k < K; ++k) {
    if (!x[k] || !g[k] || counts[k] == 0 || w[k] != w[k]) return SSG_E_BADARG;
  }
  if (!count_chunks(K, counts, (size_t)tuning.chunk, total)) return SSG_E_TOOLARGE;
  for (size_t k = 0; k < K; ++k) {
    if (unaligned(x[k], 4) || unaligned(g[k], 4) || (grad && unaligned(grad[k], 4))) return SSG_E_ALIGN;
  }
  return 0;
}

}  // namespace mcrit

static int mcrit_chunk() { return mcrit::tuning.chunk; }

static int mcrit_grid_cap() { return mcrit::tuning.grid_cap; }

static int launch_mcrit_sums(size_t K, const size_t *x, const size_t *g, const size_t *counts, const double *w, int kind,
                             float eps, void *workspace, double *sums_out, hipStream_t st) {
  using namespace mcrit;
  return for_each_launch(
      K, x, g, nullptr, counts, w, [](size_t) { return true; },
      [&](const Set &s, size_t base, bool first) {
        double *part = (double *)workspace + base;
        with_pixel_kind<true>(kind, [&](auto kd) {
          hipLaunchKernelGGL(mcrit_sums_kernel<decltype(kd)::value>, dim3(grid_of(s.n_chunks, tuning)), dim3(NT), 0, st,
                             s, eps, part);
        });
        hipLaunchKernelGGL(mcrit_fold_kernel, dim3(1), dim3(NT), 0, st, s, (int)(kind == SSG_PIX_FRO), (int)!first,
                           (const double *)part, sums_out, (int)K);
        return (int)hipGetLastError();
      });
}

static int launch_mcrit_grad(size_t K, const size_t *x, const size_t *g, const size_t *grad, const size_t *counts,
                             const double *w, int kind, float eps, const double *sums, const double *coef,
                             hipStream_t st) {
  using namespace mcrit;
  return for_each_launch(
      K, x, g, grad, counts, w, [&](size_t k) { return grad[k] != 0; },
      [&](const Set &s, size_t, bool) {
        with_pixel_kind<true>(kind, [&](auto kd) {
          hipLaunchKernelGGL(mcrit_grad_kernel<decltype(kd)::value>, dim3(grid_of(s.n_chunks, tuning)), dim3(NT), 0, st,
                             s, eps, coef, sums);
        });
        return (int)hipGetLastError();
      });
}

}  // namespace ssg

// ---- (U) the entry points: every refusal is decided here, before any launch ----
using namespace ssg;

extern "C" {

int ssg_mcrit_chunk(void) { return mcrit_chunk(); }

int ssg_mcrit_grid_cap(void) { return mcrit_grid_cap(); }

size_t ssg_mcrit_workspace_bytes(size_t n_tensors, const size_t *counts) {
  size_t total = 0;
  if (!counts || n_tensors > (size_t)INT_MAX) return 0;
  if (!mcrit::count_chunks(n_tensors, counts, (size_t)mcrit_chunk(), &total)) return 0;
  return sizeof(double) * total;
}

int ssg_mcrit_sums(size_t n_tensors, const size_t *x, const size_t *g, const size_t *counts, const double *weights,
                   int kind, float eps, void *workspace, size_t workspace_bytes, double *sums_out, ssg_stream_t stream) {
  size_t total = 0;
  if (!workspace || !sums_out) return SSG_E_BADARG;
  const int rc = mcrit::check_pairs(n_tensors, x, g, nullptr, counts, weights, kind, eps, &total);
  if (rc && rc != SSG_E_ALIGN) return rc;
  if (workspace_bytes < sizeof(double) * total) return SSG_E_WORKSPACE;
  if (rc || unaligned(workspace, 8) || unaligned(sums_out, 8)) return SSG_E_ALIGN;
  return launch_mcrit_sums(n_tensors, x, g, counts, weights, kind, eps, workspace, sums_out, (hipStream_t)stream);
}

int ssg_mcrit_grad(size_t n_tensors, const size_t *x, const size_t *g, const size_t *grad, const size_t *counts,
                   const double *weights, int kind, float eps, const double *sums, const double *coef,
                   ssg_stream_t stream) {
  size_t total = 0;
  if (!grad || !sums || !coef) return SSG_E_BADARG;
  if (const int rc = mcrit::check_pairs(n_tensors, x, g, grad, counts, weights, kind, eps, &total)) return rc;
  if (unaligned(sums, 8) || unaligned(coef, 8)) return SSG_E_ALIGN;
  return launch_mcrit_grad(n_tensors, x, g, grad, counts, weights, kind, eps, sums, coef, (hipStream_t)stream);
}

#ifdef SSG_PROFILE
// PROFILING BUILD ONLY, bound by hand in tools/perceptual_time.py (not part of include/ssg_hip.h): the chunk size (a
// multiple of 4) and grid cap that ssg_mcrit_chunk / ssg_mcrit_grid_cap, and so the workspaces sized and the launches
// made afterwards, use: the A/B of profiles/perceptual_time.txt.  The product library's two are constants.
int ssg_prof_mcrit_tuning(int chunk, int grid_cap) {
  return mcrit::tuning.set(chunk, grid_cap);
}
#endif

}  // extern "C"
