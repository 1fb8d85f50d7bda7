// BSRGAN's degradation chain as ragged-batch kernels: GAN-Based-SR/train_BSGRAN/utils/utils_blindsr.py
// (degradation_bsrgan :443-530, _nocrop :532-616, _ours_p :618-706, _plus :708-792; add_blur :335-346, add_resize
// :349-360, add_Gaussian_noise :363-377, add_speckle_noise :380-395, add_Poisson_noise :398-409).  Every image of a batch
// has its own stage order (random.sample) and its own intermediate sizes (int(sf1 * w), the 1/2 pre-scale, a / sf), so a
// launch is driven by one record per image: sizes, operation, parameters.  One launch per operation kind and stage slot.
//
// Contract (this file is compiled with -ffp-contract=off; the one fused operation, the convolution's tap, is written out).
//   images   fp32 planar (C, h, w), C in {1, 3}, at element offsets of the launch's input and output buffers (the two
//            ping-pong arenas; they may be one allocation, the fill refuses records whose ranges overlap then)
//   table    4-byte words, built and CHECKED on the host by ssg_blindsr_table_fill, resident on the device:
//              [0] n_images  [1] n_tiles  [2] family  [3] 0
//              n_images + 1 words: the first tile of every image (a prefix sum; the last word is n_tiles), padded to a
//                multiple of four words
//              n_images records of 16 words (ssg_blindsr_record)
//   mapping  a workgroup of 256 threads takes tile t = blockIdx.x, then t + gridDim.x, ... (at most GRID_CAP
//            workgroups); the image is the last one whose first tile is <= t (a binary search every lane runs alike), the
//            tile inside it is row-major.  conv / resize: a tile is 8 rows of 32 output pixels, every channel; noise: 1,024
//            pixels of the flat plane, every channel.  Every output element is written by exactly one thread, no atomics:
//            the bits do not depend on the grid, and image b of a batch has the bits of the same image run alone.
//   conv     scipy.ndimage.convolve(img, k[:, :, None], mode='mirror'): out[y, x] = sum_ij k[i, j] in[fold(y s + r - i),
//            fold(x s + r - j)], r = k / 2, fold the reflection of period 2 (n - 1) (n = 1: always 0), s the output
//            stride (img[0::s, 0::s]).  The window and its halo are folded into LDS once per channel, the taps (flipped)
//            once per tile; acc = fmaf(tap, x, acc) row by row of the window.
//   resize   cv2.resize of a float32 image, interpolation 1 | 2 | 3, as OpenCV's resize.cpp orders it: the horizontal taps
//            of a source row first, then the vertical ones; every product and every sum rounded.
//   noise    the arithmetic around the draws, listed in front of the noise kernel below.
// The launchers trust the table: ssg_blindsr_table_fill refuses a bad record before anything is uploaded.
#include <limits.h>

#include <algorithm>
#include <vector>

#include "ssg_stream.hpp"

namespace ssg {
namespace blindsr {

constexpr int NT = 256;
constexpr int TW = 32, TH = 8;                    // the output tile of conv and resize
constexpr int NOISE_TILE = 1024;                  // pixels of a noise tile: four per thread
constexpr int KMAX = 9, SMAX = 4;                 // the largest kernel and the largest output stride
constexpr int LW = (TW - 1) * SMAX + KMAX, LH = (TH - 1) * SMAX + KMAX;   // the largest folded window: 133 x 37
constexpr int GRID_CAP = stream::MAX_WG;
constexpr int HEADER_WORDS = 4, RECORD_WORDS = 16;

static_assert(sizeof(ssg_blindsr_record) == 4 * RECORD_WORDS, "the record is sixteen words");

static size_t prefix_words(size_t n) { return (n + 1 + 3) / 4 * 4; }
static size_t table_words(size_t n) { return HEADER_WORDS + prefix_words(n) + RECORD_WORDS * n; }

struct View {
  int n_images, n_tiles;
  const int *first;
  const ssg_blindsr_record *rec;
};

__device__ __forceinline__ View view_of(const int *table) {
  View v;
  v.n_images = table[0], v.n_tiles = table[1];
  v.first = table + HEADER_WORDS;
  v.rec = (const ssg_blindsr_record *)(v.first + (v.n_images + 1 + 3) / 4 * 4);
  return v;
}

// the image of tile t: the last one whose first tile is <= t (images without tiles are stepped over)
__device__ __forceinline__ int image_of(const View &v, int t) {
  int lo = 0, hi = v.n_images;   // first[lo] <= t < first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (v.first[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // a NaN passes

__device__ __forceinline__ int fold(int i, int n) {
  const int p = 2 * (n - 1);
  if (p == 0) return 0;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

// ---------------------------------------------------------------- conv ----
// one output of a K x K window at w0 (row pitch LW): the taps at constant addresses of LDS, one fmaf per tap, row by row
template <int K>
__device__ __forceinline__ float window_sum(const float *taps, const float *w0) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j < K; ++j) acc = fmaf(taps[i * K + j], w0[i * LW + j], acc);
  }
  return acc;
}

__global__ __launch_bounds__(NT) void ssg_blindsr_conv_kernel(const int *table, const float *in, float *out,
                                                               const float *pool) {
  __shared__ float win[LH * LW];
  __shared__ float taps[KMAX * KMAX];
  const View v = view_of(table);
  const int lx = threadIdx.x % TW, ly = threadIdx.x / TW;
  for (int t = blockIdx.x; t < v.n_tiles; t += gridDim.x) {
    const int b = image_of(v, t);
    const ssg_blindsr_record r = v.rec[b];
    const int lt = t - v.first[b], ty = lt / r.tiles_x, tx = lt % r.tiles_x;
    const int k = r.op, s = r.stride, rad = k / 2;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int th = min(TH, r.oh - oy0), tw = min(TW, r.ow - ox0);
    const int lh = (th - 1) * s + k, lw = (tw - 1) * s + k;
    const int y0 = oy0 * s - rad, x0 = ox0 * s - rad;
    __syncthreads();                                            // the previous tile's readers are done
    for (int i = threadIdx.x; i < k * k; i += NT) taps[i] = pool[r.pool_off + (k * k - 1 - i)];   // flipped
    for (int c = 0; c < r.C; ++c) {
      const float *src = in + (size_t)r.in_off + (size_t)c * r.h * r.w;
      if (c) __syncthreads();
      for (int yy = threadIdx.x / 64; yy < lh; yy += NT / 64) {   // a wave per row of the window: no division per element
        const float *row = src + (size_t)fold(y0 + yy, r.h) * r.w;
        for (int xx = threadIdx.x % 64; xx < lw; xx += 64) win[yy * LW + xx] = row[fold(x0 + xx, r.w)];
      }
      __syncthreads();
      if (ly < th && lx < tw) {
        const float *w0 = win + ly * s * LW + lx * s;
        float acc;
        switch (k) {
          case 3: acc = window_sum<3>(taps, w0); break;
          case 5: acc = window_sum<5>(taps, w0); break;
          case 7: acc = window_sum<7>(taps, w0); break;
          default: acc = window_sum<9>(taps, w0); break;
        }
        if (r.flags & SSG_BSR_CLIP) acc = clip01(acc);
        out[(size_t)r.out_off + ((size_t)c * r.oh + oy0 + ly) * r.ow + ox0 + lx] = acc;
      }
    }
  }
}

// ---------------------------------------------------------------- resize ----
// two or four taps of one axis: LINEAR, CUBIC, and AREA where it is not a reduction of both axes
template <int N>
struct Taps {
  int i[N];
  float w[N];
};

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ __forceinline__ void linear_taps(int d, int n, int m, bool area, Taps<2> &t) {
  const double s = (double)n / (double)m;
  int sx;
  float f;
  if (area) {
    sx = (int)floor(d * s);
    f = (float)((d + 1) - (sx + 1) / s);
    f = f <= 0.f ? 0.f : f - floorf(f);
  } else {
    f = (float)((d + 0.5) * s - 0.5);
    sx = (int)floorf(f);
    f -= sx;
  }
  if (sx < 0) f = 0.f, sx = 0;
  if (sx >= n - 1) f = 0.f, sx = n - 1;
  t.i[0] = sx, t.i[1] = clampi(sx + 1, n);
  t.w[0] = 1.f - f, t.w[1] = f;
}

__device__ __forceinline__ void cubic_taps(int d, int n, int m, Taps<4> &t) {
  const double s = (double)n / (double)m;
  float f = (float)((d + 0.5) * s - 0.5);
  const int sx = (int)floorf(f);
  f -= sx;
  const float A = -0.75f;
  t.w[0] = ((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A;
  t.w[1] = ((A + 2) * f - (A + 3)) * f * f + 1;
  t.w[2] = ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1;
  t.w[3] = 1.f - t.w[0] - t.w[1] - t.w[2];
#pragma unroll
  for (int q = 0; q < 4; ++q) t.i[q] = clampi(sx - 1 + q, n);
}

// sum_y wy (sum_x wx p[iy][ix]): a row's taps left to right, then the rows top to bottom
template <int N>
__device__ __forceinline__ float tapped(const float *p, int w, const Taps<N> &ky, const Taps<N> &kx) {
  float acc = 0.f;
#pragma unroll
  for (int y = 0; y < N; ++y) {
    const float *q = p + (size_t)ky.i[y] * w;
    float row = q[kx.i[0]] * kx.w[0];
#pragma unroll
    for (int x = 1; x < N; ++x) row += q[kx.i[x]] * kx.w[x];
    acc = y ? acc + row * ky.w[y] : row * ky.w[y];
  }
  return acc;
}

// OpenCV's area table of one destination index: sources [lo, hi), weight wh on those below a, wm on [a, b), wt above
struct Cell {
  int lo, hi, a, b;
  float wh, wm, wt;
};

__device__ __forceinline__ Cell area_cell(int d, int n, int m) {
  const double s = (double)n / (double)m;
  const double f1 = d * s, f2 = f1 + s, cw = fmin(s, n - f1);
  int a = (int)ceil(f1), b = (int)floor(f2);
  b = min(b, n - 1), a = min(a, b);
  const bool head = a - f1 > 1e-3, tail = f2 - b > 1e-3;
  const float wh = head ? (float)((a - f1) / cw) : 0.f;
  const float wt = tail ? (float)(fmin(fmin(f2 - b, 1.0), cw) / cw) : 0.f;
  return Cell{max(head ? a - 1 : a, 0), min(tail ? b + 1 : b, n), a, b, wh, (float)(1.0 / cw), wt};
}

__device__ __forceinline__ float cell_weight(const Cell c, int i) {
  const int a = c.a, b = c.b;
  const float wh = c.wh, wm = c.wm, wt = c.wt;      // (values, so that the choice is not one between addresses)
  return i < a ? wh : (i < b ? wm : wt);
}

__global__ __launch_bounds__(NT) void ssg_blindsr_resize_kernel(const int *table, const float *in, float *out) {
  const View v = view_of(table);
  const int lx = threadIdx.x % TW, ly = threadIdx.x / TW;
  for (int t = blockIdx.x; t < v.n_tiles; t += gridDim.x) {
    const int b = image_of(v, t);
    const ssg_blindsr_record &r = v.rec[b];
    const int lt = t - v.first[b], ty = lt / r.tiles_x, tx = lt % r.tiles_x;
    const int oy = ty * TH + ly, ox = tx * TW + lx;
    if (oy >= r.oh || ox >= r.ow) continue;
    const bool clip = r.flags & SSG_BSR_CLIP;
    const size_t plane = (size_t)r.h * r.w, oplane = (size_t)r.oh * r.ow;
    const float *src = in + (size_t)r.in_off;
    float *dst = out + (size_t)r.out_off + (size_t)oy * r.ow + ox;
    const bool reduce = r.h >= r.oh && r.w >= r.ow;             // both ratios >= 1
    if (r.op == SSG_BSR_AREA && reduce) {
      if (r.h % r.oh == 0 && r.w % r.ow == 0) {                 // both integer: the box mean
        const int sy = r.h / r.oh, sx = r.w / r.ow;
        const float scale = (float)(1.0 / ((double)sy * sx));
        for (int c = 0; c < r.C; ++c) {
          const float *p = src + c * plane + (size_t)oy * sy * r.w + (size_t)ox * sx;
          float sum = 0.f;
          for (int y = 0; y < sy; ++y)
            for (int x = 0; x < sx; ++x) sum += p[(size_t)y * r.w + x];
          const float o = sum * scale;
          dst[c * oplane] = clip ? clip01(o) : o;
        }
      } else {
        const Cell cy = area_cell(oy, r.h, r.oh), cx = area_cell(ox, r.w, r.ow);
        for (int c = 0; c < r.C; ++c) {
          const float *p = src + c * plane;
          float acc = 0.f;
          for (int y = cy.lo; y < cy.hi; ++y) {
            float row = 0.f;
            for (int x = cx.lo; x < cx.hi; ++x) row += p[(size_t)y * r.w + x] * cell_weight(cx, x);
            acc += cell_weight(cy, y) * row;
          }
          dst[c * oplane] = clip ? clip01(acc) : acc;
        }
      }
      continue;
    }
    if (r.op == SSG_BSR_CUBIC) {
      Taps<4> ky, kx;
      cubic_taps(oy, r.h, r.oh, ky), cubic_taps(ox, r.w, r.ow, kx);
      for (int c = 0; c < r.C; ++c) {
        const float o = tapped<4>(src + c * plane, r.w, ky, kx);
        dst[c * oplane] = clip ? clip01(o) : o;
      }
    } else {
      Taps<2> ky, kx;
      linear_taps(oy, r.h, r.oh, r.op == SSG_BSR_AREA, ky), linear_taps(ox, r.w, r.ow, r.op == SSG_BSR_AREA, kx);
      for (int c = 0; c < r.C; ++c) {
        const float o = tapped<2>(src + c * plane, r.w, ky, kx);
        dst[c * oplane] = clip ? clip01(o) : o;
      }
    }
  }
}

// ---------------------------------------------------------------- noise ----
// numpy's `np.clip((x * 255.0).round(), 0, 255) / 255.` on float32: one product, round half to even, one quotient
__device__ __forceinline__ float quantise(float x) {
  const float q = rintf(x * 255.0f);
  return (q < 0.f ? 0.f : (q > 255.f ? 255.f : q)) / 255.f;
}

// One pixel, all channels.  x: the image's planes; f: the field's (C planes, or one for the gray forms); p = r.p0.
//   GAUSS_*    y = x + fl(n p)          n = f_c | f_0 | sum_j M[c][j] f_j (the 3 x 3 matrix of the pool, C = 3)
//   SPECKLE_*  y = x + fl(x fl(n p))    x clipped first (SSG_BSR_LEAD_CLIP, as add_speckle_noise does)
//   POISSON_RATES        out_c = fl(q_c p), q = quantise(x), p = vals
//   POISSON_COLOR        y_c = fl(f_c / p)                           (f = the draw)
//   POISSON_RATES_GRAY   out_0 = (float)(g p): g = quantise in fp64 of the luminance fma(q_2, 0.114, fma(q_1, 0.587, 0.299 q_0))
//   POISSON_GRAY         y_c = (float)(q_c + (fl(f_0 / p) - g))      every operation in fp64, as numpy promotes it
// and the closing clip where SSG_BSR_CLIP is set.
__global__ __launch_bounds__(NT) void ssg_blindsr_noise_kernel(const int *table, const float *in, float *out,
                                                                const float *field, const float *pool) {
  const View v = view_of(table);
  for (int t = blockIdx.x; t < v.n_tiles; t += gridDim.x) {
    const int b = image_of(v, t);
    const ssg_blindsr_record r = v.rec[b];
    const size_t plane = (size_t)r.h * r.w;
    const size_t first = (size_t)(t - v.first[b]) * NOISE_TILE;
    const size_t last = first + NOISE_TILE < plane ? first + NOISE_TILE : plane;
    const float *x = in + (size_t)r.in_off, *f = field + (size_t)r.field_off;
    float *y = out + (size_t)r.out_off;
    const float p = r.p0;
    const bool clip = r.flags & SSG_BSR_CLIP, lead = r.flags & SSG_BSR_LEAD_CLIP;
    float M[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (r.op == SSG_BSR_GAUSS_CORR || r.op == SSG_BSR_SPECKLE_CORR) {
#pragma unroll
      for (int q = 0; q < 9; ++q) M[q] = pool[r.pool_off + q];
    }
    for (size_t e = first + threadIdx.x; e < last; e += NT) {
      float xs[3] = {0.f, 0.f, 0.f}, o[3];
      for (int c = 0; c < r.C; ++c) xs[c] = x[c * plane + e];
      int planes_out = r.C;
      switch (r.op) {
        case SSG_BSR_GAUSS_COLOR: case SSG_BSR_GAUSS_GRAY: case SSG_BSR_GAUSS_CORR:
        case SSG_BSR_SPECKLE_COLOR: case SSG_BSR_SPECKLE_GRAY: case SSG_BSR_SPECKLE_CORR: {
          float n[3];
          if (r.op == SSG_BSR_GAUSS_GRAY || r.op == SSG_BSR_SPECKLE_GRAY) {
            n[0] = n[1] = n[2] = f[e];
          } else if (r.op == SSG_BSR_GAUSS_COLOR || r.op == SSG_BSR_SPECKLE_COLOR) {
            for (int c = 0; c < r.C; ++c) n[c] = f[c * plane + e];
          } else {
            const float z0 = f[e], z1 = f[plane + e], z2 = f[2 * plane + e];
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = (M[3 * c] * z0 + M[3 * c + 1] * z1) + M[3 * c + 2] * z2;
          }
          const bool mult = r.op >= SSG_BSR_SPECKLE_COLOR;
          for (int c = 0; c < r.C; ++c) {
            const float xc = lead ? clip01(xs[c]) : xs[c], nc = n[c] * p;
            o[c] = mult ? xc + xc * nc : xc + nc;
          }
          break;
        }
        case SSG_BSR_POISSON_RATES:
          for (int c = 0; c < r.C; ++c) o[c] = quantise(xs[c]) * p;
          break;
        case SSG_BSR_POISSON_COLOR:
          for (int c = 0; c < r.C; ++c) o[c] = f[c * plane + e] / p;
          break;
        default: {                                     // the two gray forms (C = 3)
          const double q0 = quantise(xs[0]), q1 = quantise(xs[1]), q2 = quantise(xs[2]);
          const double lum = fma(q2, 0.114, fma(q1, 0.587, q0 * 0.299));   // numpy's dot: a fused chain
          const double gq = rint(lum * 255.0);
          const double g = (gq < 0.0 ? 0.0 : (gq > 255.0 ? 255.0 : gq)) / 255.0;
          if (r.op == SSG_BSR_POISSON_RATES_GRAY) {
            o[0] = (float)(g * (double)p);
            planes_out = 1;
          } else {
            const double noise = (double)(f[e] / p) - g;
            o[0] = (float)(q0 + noise), o[1] = (float)(q1 + noise), o[2] = (float)(q2 + noise);
          }
        }
      }
      for (int c = 0; c < planes_out; ++c) y[c * plane + e] = clip ? clip01(o[c]) : o[c];
    }
  }
}

// ---------------------------------------------------------------- host ----
static bool noise_op(int op) { return op >= SSG_BSR_GAUSS_COLOR && op <= SSG_BSR_POISSON_GRAY; }

// planes of the output and of the field of a noise operation on C channels
static int noise_out_planes(int op, int C) { return op == SSG_BSR_POISSON_RATES_GRAY ? 1 : C; }
static int noise_field_planes(int op, int C) {
  switch (op) {
    case SSG_BSR_GAUSS_GRAY: case SSG_BSR_SPECKLE_GRAY: case SSG_BSR_POISSON_GRAY: return 1;
    case SSG_BSR_POISSON_RATES: case SSG_BSR_POISSON_RATES_GRAY: return 0;
    default: return C;
  }
}

// the checks of one record and its tile count; 0 or a status
static int check_record(int family, const ssg_blindsr_record &r, size_t in_elems, size_t out_elems, size_t field_elems,
                        size_t pool_elems, size_t *tiles, size_t *in_n, size_t *out_n) {
  if ((r.C != 1 && r.C != 3) || r.h < 1 || r.w < 1 || r.oh < 1 || r.ow < 1) return SSG_E_BADARG;
  if (r.flags & ~(SSG_BSR_CLIP | SSG_BSR_LEAD_CLIP)) return SSG_E_BADARG;
  if ((size_t)r.C * r.h * r.w > (size_t)INT_MAX || (size_t)r.C * r.oh * r.ow > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  size_t planes_out = r.C;
  if (family == SSG_BSR_CONV) {
    if (r.op < 3 || r.op > KMAX || r.op % 2 == 0 || r.stride < 1 || r.stride > SMAX) return SSG_E_BADARG;
    if (r.oh != (r.h + r.stride - 1) / r.stride || r.ow != (r.w + r.stride - 1) / r.stride) return SSG_E_BADARG;
    if ((size_t)r.pool_off + (size_t)r.op * r.op > pool_elems) return SSG_E_WORKSPACE;
  } else if (family == SSG_BSR_RESIZE) {
    if (r.op != SSG_BSR_LINEAR && r.op != SSG_BSR_CUBIC && r.op != SSG_BSR_AREA) return SSG_E_BADARG;
  } else {
    if (!noise_op(r.op) || r.oh != r.h || r.ow != r.w || !(r.p0 == r.p0)) return SSG_E_BADARG;
    const bool corr = r.op == SSG_BSR_GAUSS_CORR || r.op == SSG_BSR_SPECKLE_CORR;
    const bool gray = r.op == SSG_BSR_POISSON_RATES_GRAY || r.op == SSG_BSR_POISSON_GRAY;
    if ((corr || gray) && r.C != 3) return SSG_E_BADARG;
    if (corr && (size_t)r.pool_off + 9 > pool_elems) return SSG_E_WORKSPACE;
    if ((size_t)r.field_off + (size_t)noise_field_planes(r.op, r.C) * r.h * r.w > field_elems) return SSG_E_WORKSPACE;
    planes_out = noise_out_planes(r.op, r.C);
  }
  *in_n = (size_t)r.C * r.h * r.w, *out_n = planes_out * r.oh * r.ow;
  if ((size_t)r.in_off + *in_n > in_elems || (size_t)r.out_off + *out_n > out_elems) return SSG_E_WORKSPACE;
  if (family == SSG_BSR_NOISE) *tiles = ((size_t)r.h * r.w + NOISE_TILE - 1) / NOISE_TILE;
  else *tiles = (size_t)((r.oh + TH - 1) / TH) * ((r.ow + TW - 1) / TW);
  return 0;
}

}  // namespace blindsr

static int blindsr_grid_cap() { return blindsr::GRID_CAP; }

static int launch_blindsr(int family, const void *table, int n_tiles, const float *in, float *out, const float *field,
                          const float *pool, hipStream_t st) {
  using namespace blindsr;
  const dim3 grid((unsigned)std::min(n_tiles, GRID_CAP)), block(NT);
  const int *tab = (const int *)table;
  if (family == SSG_BSR_CONV) hipLaunchKernelGGL(ssg_blindsr_conv_kernel, grid, block, 0, st, tab, in, out, pool);
  else if (family == SSG_BSR_RESIZE) hipLaunchKernelGGL(ssg_blindsr_resize_kernel, grid, block, 0, st, tab, in, out);
  else hipLaunchKernelGGL(ssg_blindsr_noise_kernel, grid, block, 0, st, tab, in, out, field, pool);
  return (int)hipGetLastError();
}

}  // namespace ssg

// ---- (T) the entry points: every refusal is decided here, before the launch ----
using namespace ssg;

extern "C" {

int ssg_blindsr_grid_cap(void) { return blindsr_grid_cap(); }

int ssg_blindsr_tile(int family, int *tile_rows, int *tile_cols) {
  if (family < SSG_BSR_CONV || family > SSG_BSR_NOISE || !tile_rows || !tile_cols) return SSG_E_BADARG;
  *tile_rows = family == SSG_BSR_NOISE ? 1 : blindsr::TH;
  *tile_cols = family == SSG_BSR_NOISE ? blindsr::NOISE_TILE : blindsr::TW;
  return 0;
}

size_t ssg_blindsr_table_bytes(int n_images) {
  return n_images < 0 ? 0 : sizeof(int) * blindsr::table_words((size_t)n_images);
}

int ssg_blindsr_table_fill(int family, const ssg_blindsr_record *records, int n_images, size_t in_elems,
                           size_t out_elems, size_t field_elems, size_t pool_elems, int same_buffer, void *table,
                           size_t table_bytes, int *n_tiles_out) {
  using namespace blindsr;
  if (family < SSG_BSR_CONV || family > SSG_BSR_NOISE || n_images < 0 || !table || !n_tiles_out) return SSG_E_BADARG;
  if (n_images && !records) return SSG_E_BADARG;
  if (unaligned(table, sizeof(int))) return SSG_E_ALIGN;
  if (in_elems > (size_t)UINT_MAX || out_elems > (size_t)UINT_MAX || field_elems > (size_t)UINT_MAX ||
      pool_elems > (size_t)UINT_MAX)
    return SSG_E_TOOLARGE;
  if (table_bytes < sizeof(int) * table_words((size_t)n_images)) return SSG_E_WORKSPACE;
  int *words = (int *)table, *first = words + HEADER_WORDS;
  ssg_blindsr_record *rec = (ssg_blindsr_record *)(first + prefix_words((size_t)n_images));
  std::vector<std::pair<size_t, size_t>> reads, writes;      // [begin, end) of every image's input and output
  size_t total = 0;
  for (int i = 0; i < n_images; ++i) {
    size_t tiles = 0, in_n = 0, out_n = 0;
    const int status = check_record(family, records[i], in_elems, out_elems, field_elems, pool_elems, &tiles, &in_n, &out_n);
    if (status) return status;
    if (total + tiles > (size_t)INT_MAX) return SSG_E_TOOLARGE;
    reads.emplace_back(records[i].in_off, records[i].in_off + in_n);
    writes.emplace_back(records[i].out_off, records[i].out_off + out_n);
    first[i] = (int)total;
    total += tiles;
  }
  // no output may overlap another output, nor (in one buffer) any input: each element has one writer and no late reader
  std::sort(writes.begin(), writes.end());
  for (size_t i = 1; i < writes.size(); ++i)
    if (writes[i].first < writes[i - 1].second) return SSG_E_BADARG;
  if (same_buffer) {
    std::sort(reads.begin(), reads.end());
    size_t j = 0, furthest = 0;                                // the furthest end of the reads that begin before a write
    for (const auto &wr : writes) {
      for (; j < reads.size() && reads[j].first < wr.second; ++j) furthest = std::max(furthest, reads[j].second);
      if (furthest > wr.first) return SSG_E_BADARG;
    }
  }
  words[0] = n_images, words[1] = (int)total, words[2] = family, words[3] = 0;
  for (size_t i = (size_t)n_images; i < prefix_words((size_t)n_images); ++i) first[i] = (int)total;
  for (int i = 0; i < n_images; ++i) {
    rec[i] = records[i];
    rec[i].tile0 = first[i];
    rec[i].tiles_x = family == SSG_BSR_NOISE ? 1 : (records[i].ow + TW - 1) / TW;
    rec[i].reserved = 0;
  }
  *n_tiles_out = (int)total;
  return 0;
}

static int blindsr_apply(int family, const void *table, int n_tiles, const float *in, float *out, const float *field,
                         const float *pool, ssg_stream_t stream) {
  if (!table || !in || !out || n_tiles < 0) return SSG_E_BADARG;
  if (unaligned(table, sizeof(int)) || unaligned(in, sizeof(float)) || unaligned(out, sizeof(float)) ||
      unaligned(field, sizeof(float)) || unaligned(pool, sizeof(float)))
    return SSG_E_ALIGN;
  if (n_tiles == 0) return 0;
  return launch_blindsr(family, table, n_tiles, in, out, field, pool, (hipStream_t)stream);
}

int ssg_blindsr_conv(const void *table, int n_tiles, const float *in, float *out, const float *pool,
                     ssg_stream_t stream) {
  if (!pool) return SSG_E_BADARG;
  return blindsr_apply(SSG_BSR_CONV, table, n_tiles, in, out, nullptr, pool, stream);
}

int ssg_blindsr_resize(const void *table, int n_tiles, const float *in, float *out, ssg_stream_t stream) {
  return blindsr_apply(SSG_BSR_RESIZE, table, n_tiles, in, out, nullptr, nullptr, stream);
}

int ssg_blindsr_noise(const void *table, int n_tiles, const float *in, float *out, const float *field,
                      const float *pool, ssg_stream_t stream) {
  return blindsr_apply(SSG_BSR_NOISE, table, n_tiles, in, out, field, pool, stream);
}

}  // extern "C"
