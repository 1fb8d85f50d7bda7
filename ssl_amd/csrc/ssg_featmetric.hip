// The criteria of the two feature-space validation metrics outside their networks, over a RAGGED SET of feature pairs in
// one launch each: LPIPS v0.1 (normalise both maps over channels, square the difference, 1x1 convolution, spatial mean,
// per tapped layer) and DISTS (five moments per channel plane, the structure and texture terms, the weighted sum).  The
// pairs differ in size by up to 256 : 1; every one is read ONCE, and nothing of feature size is written.
//
// Contract (this file is compiled with -ffp-contract=off).  Inputs are fp32 NCHW contiguous, N images to a layer, and
// need only a float's alignment.  Every sum is fp64, of products of two fp32 factors formed in fp64 (so exact), in a
// fixed order: no atomics, no tickets, no scratch; one partial per work unit in the workspace, folded in unit order.
//
//   ssg_lpips_layers   layer k = (f0, f1, w, C, H, W).  Per pixel, in ONE pass over the channels, the five sums
//            P0 = sum f0^2, P1 = sum f1^2, A = sum w f0^2, Cc = sum w f1^2, B = sum w f0 f1, then with i = 1 / (sqrt(P) +
//            1e-10):  d = ((A i0) i0 - 2 ((B i0) i1)) + (Cc i1) i1, and 0 where that is negative.  Identical inputs give
//            the three terms t, 2 t, t and so exactly 0; an all-zero vector gives i = 1e10 and zero sums, so the
//            package's 0 / (0 + eps) = 0.  A NaN passes through (the clamp is a comparison).
//   ssg_lpips_layers_backward   the adjoint of the UNCLAMPED d with respect to both maps, in ONE launch for all layers
//            and both sides, with the forward's units.  Pass 1 forms the five sums exactly as above; slice 0 turns them
//            into the pixel's six scalars (n = sqrt(P), i = 1 / (n + 1e-10), s = coef[n] / HW)
//              i0, i1, q0 = (A i0 - B i1) (i0 / n0), q1 = (Cc i1 - B i0) (i1 / n1), m0 = (2 s) i0, m1 = (2 s) i1
//            and hands them to every slice through LDS; pass 2 walks the slice's channels again (the second read is
//            meant to hit L2) and stores g0_c = m0 (w_c (f0_c i0 - f1_c i1) - q0 f0_c), g1_c = m1 (w_c (f1_c i1 - f0_c i0)
//            - q1 f1_c), every operation fp64 and one cast at the store, consecutive lanes to consecutive addresses.
//            Identical inputs: f0 i0 - f1 i1 and A i0 - B i1 are differences of equal numbers, so every element is +-0.
//            An all-zero vector (n = 0): q = 0 * inf = NaN on THAT side's C elements of the pixel, as torch's lines give
//            (0 * inf in sqrt's backward); the other side stays finite.  One writer per element, no workspace.
//            A work unit is px pixels of one image of one layer, px = the power of two at or above min(HW, 256); the 256
//            threads are px pixel lanes (consecutive addresses along HW: coalesced) times 256 / px channel slices
//            (slice s takes channels s, s + 256 / px, ...).  At HW >= 256 a thread owns one pixel and walks all C
//            channels; at HW = 9 sixteen slices share each pixel.  The slices' sums are added through LDS in slice
//            order, the unit's d are folded as ssg_stream.hpp folds, and ONE double per unit goes to the workspace.  The
//            fold launch (one workgroup per image) adds a layer's units in order (thread i takes i, i + 256, ..., then an
//            LDS tree), divides by HW and adds the layers in order: out[n][k], k < K, and out[n][K] their sum.
//            The geometry of a layer depends on its HW alone, so its partials are the same bits whichever other layers
//            and images are in the call.
//   ssg_dists_score    layer k = (x, y, C, H, W).  A chunk is featmetric_chunk() elements of ONE plane (ssg_chunked.hpp's
//            span; the walk is this file's own, see the kernel); per chunk the five sums sum x, sum y, sum x^2, sum y^2, sum x y as 5 doubles in the workspace at
//            5 * chunk, chunks ordered layer, image, channel, chunk of the plane.  The finish launch (one workgroup per
//            image) folds a plane's chunks in order, forms mx = Sx / HW, vx = Sxx / HW - mx mx, cov = Sxy / HW - mx my,
//            S1 = (2 mx my + c1) / (mx mx + my my + c1), S2 = (2 cov + c2) / (vx + vy + c2), c1 = c2 = 1e-6, and adds
//            alpha_c S1, beta_c S2 and alpha_c, beta_c over all channels in a fixed order (thread t takes channels t, t +
//            256, ... of each layer in layer order, then an LDS tree): out[n] = {1 - (s1 + s2) / ws, s1 / ws, s2 / ws},
//            ws = sum alpha + sum beta.  A one-element plane has vx = cov = 0 exactly, so S2 = 1.
// The layer records travel BY VALUE in the kernels' arguments (feature maps move from call to call).  Both main kernels
// run under a grid cap with a grid-stride loop.  The launchers trust their arguments: the entry points below refuse.
#include "ssg_chunked.hpp"

namespace ssg {
namespace featmetric {

using namespace chunked;

constexpr int UNIT = NT;           // LPIPS: pixels per work unit at HW >= 256 (one per thread)
constexpr int CHUNK = 8192;        // DISTS: elements per chunk (ssg_mcrit.hip's, the same walk)
constexpr int GRID_CAP = MAX_WG;   // four workgroups per CU
constexpr int MAX_LAYERS = 16;

struct LpipsLayer {
  const float *f0, *f1, *w;
  unsigned C, HW;
  unsigned first;    // the layer's first unit
  unsigned units;    // units per image
  unsigned px_log2;  // pixel lanes per unit = 1 << px_log2
};

struct LpipsSet {
  LpipsLayer l[MAX_LAYERS];
  int K, N;
  unsigned n_units;
};

struct LpipsGradLayer {
  const float *f0, *f1, *w;
  float *g0, *g1;    // either null for the whole set: that side wants no gradient
  unsigned C, HW;
  unsigned first, units, px_log2;   // as LpipsLayer's
};

struct LpipsGradSet {
  LpipsGradLayer l[MAX_LAYERS];
  int K, N;
  unsigned n_units;
  const float *coef;   // N: the upstream gradient of out[n][K]
};

struct DistsLayer {
  const float *x, *y;
  unsigned C, HW;
  unsigned first;    // the layer's first chunk
  unsigned cpp;      // chunks per plane
  unsigned ch0;      // the layer's first channel in alpha / beta
};

struct DistsSet {
  DistsLayer l[MAX_LAYERS];
  int K, N;
  unsigned n_chunks;
};

// the layer of a work unit, by compare and select over the records (kernel arguments: no table in memory)
template <class Set>
__device__ __forceinline__ auto layer_of(const Set &s, unsigned u) {
  auto cur = s.l[0];
#pragma unroll
  for (int k = 1; k < MAX_LAYERS; ++k) {
    if (k < s.K && u >= s.l[k].first) cur = s.l[k];
  }
  return cur;
}

__global__ __launch_bounds__(NT) void lpips_kernel(const LpipsSet s, double *part) {
  __shared__ double sh[5][NT];
  const unsigned t = threadIdx.x;
  for (unsigned unit = blockIdx.x; unit < s.n_units; unit += gridDim.x) {
    const LpipsLayer l = layer_of(s, unit);
    const unsigned rel = unit - l.first, n = rel / l.units, u = rel % l.units;
    const unsigned px = 1u << l.px_log2, cs = NT >> l.px_log2;
    const unsigned lane = t & (px - 1), slice = t >> l.px_log2;
    const size_t pix = (size_t)u * px + lane;
    const bool live = pix < l.HW;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
      const size_t base = (size_t)n * l.C * l.HW + pix;
      const float *p0 = l.f0 + base, *p1 = l.f1 + base;
#pragma unroll 4
      for (unsigned c = slice; c < l.C; c += cs) {
        const size_t o = (size_t)c * l.HW;
        const double x = (double)p0[o], y = (double)p1[o], w = (double)l.w[c];
        const double xx = x * x, yy = y * y, xy = x * y;
        a[0] += xx, a[1] += yy, a[2] += w * xx, a[3] += w * yy, a[4] += w * xy;
      }
    }
    if (cs > 1) {   // (uniform over the workgroup: the layer's geometry)
#pragma unroll
      for (int j = 0; j < 5; ++j) sh[j][t] = a[j];
      __syncthreads();
      if (slice == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          double r = sh[j][lane];
          for (unsigned q = 1; q < cs; ++q) r += sh[j][q * px + lane];
          a[j] = r;
        }
      }
    }
    double d = 0.0;
    if (live && slice == 0) {
      const double i0 = 1.0 / (sqrt(a[0]) + 1e-10), i1 = 1.0 / (sqrt(a[1]) + 1e-10);
      const double t0 = (a[2] * i0) * i0, t1 = 2.0 * ((a[4] * i0) * i1), t2 = (a[3] * i1) * i1;
      d = (t0 - t1) + t2;
      d = d < 0.0 ? 0.0 : d;   // (a NaN fails the comparison and stays)
    }
    workgroup_fold<1>({d}, part + unit);
    __syncthreads();   // (sh and the fold's LDS words are written again in the next trip)
  }
}

// one workgroup per image: out[n][k] = (sum of the layer's units) / HW, out[n][K] = their sum in layer order
__global__ __launch_bounds__(NT) void lpips_fold_kernel(const LpipsSet s, const double *part, double *out) {
  __shared__ double sh[NT];
  const unsigned t = threadIdx.x, n = blockIdx.x;
  double total = 0.0;
  for (int k = 0; k < s.K; ++k) {
    const LpipsLayer &l = s.l[k];
    const double *p = part + l.first + (size_t)n * l.units;
    double a = 0.0;
    for (unsigned i = t; i < l.units; i += NT) a += p[i];
    sh[t] = a;
    __syncthreads();
    for (unsigned o = NT / 2; o > 0; o >>= 1) {
      if (t < o) sh[t] += sh[t + o];
      __syncthreads();
    }
    if (t == 0) {
      const double v = sh[0] / (double)l.HW;
      out[(size_t)n * (s.K + 1) + k] = v;
      total += v;
    }
    __syncthreads();
  }
  if (t == 0) out[(size_t)n * (s.K + 1) + s.K] = total;
}

// the adjoint of lpips_kernel's unclamped d: the same units, the same five sums, then a second walk that stores
__global__ __launch_bounds__(NT) void lpips_grad_kernel(const LpipsGradSet s) {
  __shared__ double sh[6][NT];
  const unsigned t = threadIdx.x;
  for (unsigned unit = blockIdx.x; unit < s.n_units; unit += gridDim.x) {
    const LpipsGradLayer l = layer_of(s, unit);
    const unsigned rel = unit - l.first, n = rel / l.units, u = rel % l.units;
    const unsigned px = 1u << l.px_log2, cs = NT >> l.px_log2;
    const unsigned lane = t & (px - 1), slice = t >> l.px_log2;
    const size_t pix = (size_t)u * px + lane;
    const bool live = pix < l.HW;
    const size_t base = (size_t)n * l.C * l.HW + pix;
    const float *p0 = l.f0 + base, *p1 = l.f1 + base;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
#pragma unroll 4
      for (unsigned c = slice; c < l.C; c += cs) {
        const size_t o = (size_t)c * l.HW;
        const double x = (double)p0[o], y = (double)p1[o], w = (double)l.w[c];
        const double xx = x * x, yy = y * y, xy = x * y;
        a[0] += xx, a[1] += yy, a[2] += w * xx, a[3] += w * yy, a[4] += w * xy;
      }
    }
    if (cs > 1) {   // (uniform over the workgroup: the layer's geometry)
#pragma unroll
      for (int j = 0; j < 5; ++j) sh[j][t] = a[j];
      __syncthreads();
      if (slice == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          double r = sh[j][lane];
          for (unsigned q = 1; q < cs; ++q) r += sh[j][q * px + lane];
          a[j] = r;
        }
      }
    }
    // the pixel's scalars, by slice 0 alone (the only slice where cs = 1).  A dead lane's sums are 0, so its q are
    // 0 * inf = NaN: they are handed round like the others and never used, pass 2 skips a dead lane.
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (slice == 0) {
      const double n0 = sqrt(a[0]), n1 = sqrt(a[1]);
      const double i0 = 1.0 / (n0 + 1e-10), i1 = 1.0 / (n1 + 1e-10);
      const double sc = 2.0 * ((double)s.coef[n] / (double)l.HW);
      v[0] = i0, v[1] = i1;
      v[2] = (a[2] * i0 - a[4] * i1) * (i0 / n0);
      v[3] = (a[3] * i1 - a[4] * i0) * (i1 / n1);
      v[4] = sc * i0, v[5] = sc * i1;
    }
    if (cs > 1) {
      // (slice 0 of a lane is the only reader of that lane's columns above, so it may overwrite column `lane` here)
      if (slice == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) sh[j][lane] = v[j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 6; ++j) v[j] = sh[j][lane];
    }
    if (live) {
      float *q0 = l.g0 ? l.g0 + base : nullptr, *q1 = l.g1 ? l.g1 + base : nullptr;
#pragma unroll 4
      for (unsigned c = slice; c < l.C; c += cs) {
        const size_t o = (size_t)c * l.HW;
        const double x = (double)p0[o], y = (double)p1[o], w = (double)l.w[c];
        const double xn = x * v[0], yn = y * v[1];
        if (q0) q0[o] = (float)(v[4] * (w * (xn - yn) - v[2] * x));
        if (q1) q1[o] = (float)(v[5] * (w * (yn - xn) - v[3] * y));
      }
    }
    if (cs > 1) __syncthreads();   // (sh is written again in the next trip)
  }
}

__global__ __launch_bounds__(NT) void dists_moments_kernel(const DistsSet s, double *part) {
  for (unsigned c = blockIdx.x; c < s.n_chunks; c += gridDim.x) {
    const DistsLayer l = layer_of(s, c);
    const unsigned rel = c - l.first;
    const size_t plane = rel / l.cpp;   // n C + channel
    const Span sp = span_of(l.HW, rel % l.cpp, CHUNK);
    const float *x = l.x + plane * l.HW + sp.off, *y = l.y + plane * l.HW + sp.off;
    // NOT ssg_chunked.hpp's walk: its head / quads / tail split follows the address, and with it which thread adds which
    // element.  Here thread t takes the groups t, t + 256, ... of four elements counted from the chunk's start and then
    // the tail, whatever the alignment, so a plane's sums are the same bits wherever it lies (image n of a batch and
    // the image alone lie at different offsets mod 16 whenever C H W is odd); only the width of the loads follows it.
    const bool xv = ((size_t)x & 15) == 0, yv = ((size_t)y & 15) == 0;
    const unsigned n4 = sp.len / EPT;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    auto add = [&](float xf, float yf) {
      const double a = (double)xf, b = (double)yf;
      m[0] += a, m[1] += b, m[2] += a * a, m[3] += b * b, m[4] += a * b;
    };
    for (unsigned q = threadIdx.x; q < n4; q += NT) {
      float a[4], b[4];
      load4(x + EPT * q, xv, a);
      load4(y + EPT * q, yv, b);
      for (int k = 0; k < 4; ++k) add(a[k], b[k]);
    }
    for (unsigned e = EPT * n4 + threadIdx.x; e < sp.len; e += NT) add(x[e], y[e]);
    workgroup_fold<5>(m, part + 5 * (size_t)c);
    __syncthreads();   // (the fold's LDS words are written again in the next trip)
  }
}

// one workgroup per image: the planes' moments from their chunks, S1 and S2, the weighted sums over all channels
__global__ __launch_bounds__(NT) void dists_finish_kernel(const DistsSet s, const double *part, const float *alpha,
                                                          const float *beta, double *out) {
  __shared__ double sh[3][NT];
  const unsigned t = threadIdx.x, n = blockIdx.x;
  const double c1 = 1e-6, c2 = 1e-6;
  double s1 = 0.0, s2 = 0.0, ws = 0.0;
  for (int k = 0; k < s.K; ++k) {
    const DistsLayer &l = s.l[k];
    const double hw = (double)l.HW;
    for (unsigned c = t; c < l.C; c += NT) {
      const double *p = part + 5 * ((size_t)l.first + ((size_t)n * l.C + c) * l.cpp);
      double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (unsigned j = 0; j < l.cpp; ++j) {
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] += p[5 * (size_t)j + q];
      }
      const double mx = m[0] / hw, my = m[1] / hw;
      const double vx = m[2] / hw - mx * mx, vy = m[3] / hw - my * my, cov = m[4] / hw - mx * my;
      const double S1 = (2.0 * mx * my + c1) / ((mx * mx + my * my) + c1);
      const double S2 = (2.0 * cov + c2) / ((vx + vy) + c2);
      const double a = (double)alpha[l.ch0 + c], b = (double)beta[l.ch0 + c];
      s1 += a * S1, s2 += b * S2, ws += a + b;
    }
  }
  sh[0][t] = s1, sh[1][t] = s2, sh[2][t] = ws;
  __syncthreads();
  for (unsigned o = NT / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int q = 0; q < 3; ++q) sh[q][t] += sh[q][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double d1 = sh[0][0] / sh[2][0], d2 = sh[1][0] / sh[2][0];
    out[3 * (size_t)n] = 1.0 - (d1 + d2);
    out[3 * (size_t)n + 1] = d1;
    out[3 * (size_t)n + 2] = d2;
  }
}

// ---- host ----
// what both entry points check of the shapes: K, N, C, H, W; fills hw[k]
static int check_shapes(int K, int N, const int *C, const int *H, const int *W, size_t *hw) {
  if (K < 1 || K > MAX_LAYERS || N < 1 || !C || !H || !W) return SSG_E_BADARG;
  for (int k = 0; k < K; ++k) {
    if (C[k] < 1 || H[k] < 1 || W[k] < 1) return SSG_E_BADARG;
    hw[k] = (size_t)H[k] * (size_t)W[k];
    if (hw[k] > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  }
  return 0;
}

inline unsigned px_log2_of(size_t hw) {
  unsigned b = 0;
  while (b < 8 && ((size_t)1 << b) < hw) ++b;   // the power of two at or above min(HW, 256)
  return b;
}

// fills the shapes' part of an LPIPS set (no pointers); SSG_E_TOOLARGE where the unit count leaves an int
static int lpips_plan(int K, int N, const int *C, const int *H, const int *W, LpipsSet *s) {
  size_t hw[MAX_LAYERS], total = 0;
  if (const int rc = check_shapes(K, N, C, H, W, hw)) return rc;
  s->K = K, s->N = N;
  for (int k = 0; k < K; ++k) {
    LpipsLayer &l = s->l[k];
    l.f0 = l.f1 = l.w = nullptr;
    l.C = (unsigned)C[k], l.HW = (unsigned)hw[k], l.px_log2 = px_log2_of(hw[k]);
    l.units = (unsigned)chunks_of(hw[k], (size_t)1 << l.px_log2);
    l.first = (unsigned)total;
    total += (size_t)N * l.units;
    if (total > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  }
  for (int k = K; k < MAX_LAYERS; ++k) s->l[k] = s->l[0];   // (never selected: defined bytes for the launch)
  s->n_units = (unsigned)total;
  return 0;
}

static int dists_plan(int K, int N, const int *C, const int *H, const int *W, DistsSet *s) {
  size_t hw[MAX_LAYERS], total = 0, channels = 0;
  if (const int rc = check_shapes(K, N, C, H, W, hw)) return rc;
  s->K = K, s->N = N;
  for (int k = 0; k < K; ++k) {
    DistsLayer &l = s->l[k];
    l.x = l.y = nullptr;
    l.C = (unsigned)C[k], l.HW = (unsigned)hw[k], l.cpp = (unsigned)chunks_of(hw[k], CHUNK);
    l.first = (unsigned)total, l.ch0 = (unsigned)channels;
    channels += l.C;
    if ((size_t)N * l.C > (size_t)INT_MAX / l.cpp || channels > (size_t)INT_MAX) return SSG_E_TOOLARGE;
    total += (size_t)N * l.C * l.cpp;
    if (total > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  }
  for (int k = K; k < MAX_LAYERS; ++k) s->l[k] = s->l[0];
  s->n_chunks = (unsigned)total;
  return 0;
}

constexpr Tuning tuning = {CHUNK, GRID_CAP};

}  // namespace featmetric

static int featmetric_grid_cap() { return featmetric::GRID_CAP; }
static int featmetric_unit() { return featmetric::UNIT; }
static int featmetric_chunk() { return featmetric::CHUNK; }

static int launch_lpips_layers(const featmetric::LpipsSet &s, void *workspace, double *out, hipStream_t st) {
  using namespace featmetric;
  hipLaunchKernelGGL(lpips_kernel, dim3(grid_of(s.n_units, tuning)), dim3(NT), 0, st, s, (double *)workspace);
  hipLaunchKernelGGL(lpips_fold_kernel, dim3((unsigned)s.N), dim3(NT), 0, st, s, (const double *)workspace, out);
  return (int)hipGetLastError();
}

static int launch_lpips_layers_backward(const featmetric::LpipsGradSet &s, hipStream_t st) {
  using namespace featmetric;
  hipLaunchKernelGGL(lpips_grad_kernel, dim3(grid_of(s.n_units, tuning)), dim3(NT), 0, st, s);
  return (int)hipGetLastError();
}

static int launch_dists_score(const featmetric::DistsSet &s, const float *alpha, const float *beta, void *workspace, double *out,
                              hipStream_t st) {
  using namespace featmetric;
  hipLaunchKernelGGL(dists_moments_kernel, dim3(grid_of(s.n_chunks, tuning)), dim3(NT), 0, st, s, (double *)workspace);
  hipLaunchKernelGGL(dists_finish_kernel, dim3((unsigned)s.N), dim3(NT), 0, st, s, (const double *)workspace, alpha,
                     beta, out);
  return (int)hipGetLastError();
}

}  // namespace ssg

// ---- (V) the entry points: every refusal is decided here, before any launch ----
using namespace ssg;

extern "C" {

int ssg_featmetric_grid_cap(void) { return featmetric_grid_cap(); }

int ssg_featmetric_unit(void) { return featmetric_unit(); }

int ssg_featmetric_chunk(void) { return featmetric_chunk(); }

size_t ssg_lpips_workspace_bytes(int n_layers, int n_images, const int *C, const int *H, const int *W) {
  featmetric::LpipsSet s;
  if (featmetric::lpips_plan(n_layers, n_images, C, H, W, &s)) return 0;
  return sizeof(double) * (size_t)s.n_units;
}

int ssg_lpips_layers(int n_layers, int n_images, const size_t *f0, const size_t *f1, const size_t *w, const int *C,
                     const int *H, const int *W, void *workspace, size_t workspace_bytes, double *out,
                     ssg_stream_t stream) {
  using namespace featmetric;
  LpipsSet s;
  if (!f0 || !f1 || !w || !workspace || !out) return SSG_E_BADARG;
  if (const int rc = lpips_plan(n_layers, n_images, C, H, W, &s)) return rc;
  for (int k = 0; k < s.K; ++k) {
    if (!f0[k] || !f1[k] || !w[k]) return SSG_E_BADARG;
  }
  if (workspace_bytes < sizeof(double) * (size_t)s.n_units) return SSG_E_WORKSPACE;
  if (unaligned(workspace, 8) || unaligned(out, 8)) return SSG_E_ALIGN;
  for (int k = 0; k < s.K; ++k) {
    if (unaligned(f0[k], 4) || unaligned(f1[k], 4) || unaligned(w[k], 4)) return SSG_E_ALIGN;
    s.l[k].f0 = (const float *)f0[k], s.l[k].f1 = (const float *)f1[k], s.l[k].w = (const float *)w[k];
  }
  return launch_lpips_layers(s, workspace, out, (hipStream_t)stream);
}

int ssg_lpips_layers_backward(int n_layers, int n_images, const size_t *f0, const size_t *f1, const size_t *w, const int *C,
                              const int *H, const int *W, const float *coef, const size_t *grad0, const size_t *grad1,
                              ssg_stream_t stream) {
  using namespace featmetric;
  LpipsSet p;
  LpipsGradSet s;
  if (!f0 || !f1 || !w || !coef || (!grad0 && !grad1)) return SSG_E_BADARG;
  if (const int rc = lpips_plan(n_layers, n_images, C, H, W, &p)) return rc;
  for (int k = 0; k < p.K; ++k) {
    if (!f0[k] || !f1[k] || !w[k] || (grad0 && !grad0[k]) || (grad1 && !grad1[k])) return SSG_E_BADARG;
  }
  if (unaligned(coef, 4)) return SSG_E_ALIGN;
  for (int k = 0; k < p.K; ++k) {
    if (unaligned(f0[k], 4) || unaligned(f1[k], 4) || unaligned(w[k], 4) || (grad0 && unaligned(grad0[k], 4)) ||
        (grad1 && unaligned(grad1[k], 4)))
      return SSG_E_ALIGN;
  }
  s.K = p.K, s.N = p.N, s.n_units = p.n_units, s.coef = coef;
  for (int k = 0; k < MAX_LAYERS; ++k) {
    const int j = k < p.K ? k : 0;   // (beyond K: never selected, defined bytes for the launch)
    const LpipsLayer &q = p.l[j];
    LpipsGradLayer &l = s.l[k];
    l.f0 = (const float *)f0[j], l.f1 = (const float *)f1[j], l.w = (const float *)w[j];
    l.g0 = grad0 ? (float *)grad0[j] : nullptr, l.g1 = grad1 ? (float *)grad1[j] : nullptr;
    l.C = q.C, l.HW = q.HW, l.first = q.first, l.units = q.units, l.px_log2 = q.px_log2;
  }
  return launch_lpips_layers_backward(s, (hipStream_t)stream);
}

size_t ssg_dists_workspace_bytes(int n_layers, int n_images, const int *C, const int *H, const int *W) {
  featmetric::DistsSet s;
  if (featmetric::dists_plan(n_layers, n_images, C, H, W, &s)) return 0;
  return 5 * sizeof(double) * (size_t)s.n_chunks;
}

int ssg_dists_score(int n_layers, int n_images, const size_t *x, const size_t *y, const int *C, const int *H,
                    const int *W, const float *alpha, const float *beta, void *workspace, size_t workspace_bytes,
                    double *out, ssg_stream_t stream) {
  using namespace featmetric;
  DistsSet s;
  if (!x || !y || !alpha || !beta || !workspace || !out) return SSG_E_BADARG;
  if (const int rc = dists_plan(n_layers, n_images, C, H, W, &s)) return rc;
  for (int k = 0; k < s.K; ++k) {
    if (!x[k] || !y[k]) return SSG_E_BADARG;
  }
  if (workspace_bytes < 5 * sizeof(double) * (size_t)s.n_chunks) return SSG_E_WORKSPACE;
  if (unaligned(workspace, 8) || unaligned(out, 8) || unaligned(alpha, 4) ||
      unaligned(beta, 4))
    return SSG_E_ALIGN;
  for (int k = 0; k < s.K; ++k) {
    if (unaligned(x[k], 4) || unaligned(y[k], 4)) return SSG_E_ALIGN;
    s.l[k].x = (const float *)x[k], s.l[k].y = (const float *)y[k];
  }
  return launch_dists_score(s, alpha, beta, workspace, out, (hipStream_t)stream);
}

}  // extern "C"
