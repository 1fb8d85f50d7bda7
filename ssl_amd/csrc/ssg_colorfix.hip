// StableSR's colour correction of a diffusion sample on the GPU: scripts/wavelet_color_fix.py of the Diffusion fork
// (wavelet_blur :73-92, wavelet_decomposition :94-106, wavelet_reconstruction :108-119, calc_mean_std :44-57,
// adaptive_instance_normalization :59-71) and the clamp((x + 1) / 2, 0, 1) / 255 x -> byte that follows it in every
// caller (test.py:322-346).  fp32 contiguous NCHW, any B, C, H, W >= 1, planes independent; nothing is copied to the host.
//
// Contract (this file is compiled with -ffp-contract=off):
//   blur      level i = 1 .. levels has radius r = 2^(i-1) and the taps [1/4, 1/2, 1/4] per axis at -r, 0, +r, the tap
//             COORDINATE clamped to the plane at every level (replicate padding by r, then the dilated 3 x 3
//             convolution): t = 0.25 (v[x-r] + v[x+r]) + 0.5 v[x] along the rows, then the same along the columns.  The
//             taps are powers of two: only the two adds per axis round.
//   low       the image after `levels` blurs; high = image - low (the reference's sum of the per-level differences
//             telescopes to this in real arithmetic).
//   wavelet   out = content + low(style - content).  The blur is linear and clamps both images alike, so this IS
//             high(content) + low(style) in real arithmetic, with one tile pass instead of two.
//   stats     per plane K = its first element, S0 = sum x, S1 = sum (x - K), S2 = sum (x - K)^2 in fp64 over chunks of
//             4,096 elements (thread t of 256 takes elements t, t + 256, ...; pixel::block_sum), the chunks folded by
//             one workgroup per plane (thread t takes chunks t, t + 256, ... in order; block_sum): mean = S0 / n,
//             std = sqrt((S2 - S1^2 / n) / (n - 1) + eps).  n = 1 gives 0 / 0 = NaN, as torch's unbiased variance.
//             The shift makes a flat plane's variance exactly 0 and keeps the subtraction from cancelling; the mean
//             comes from the plain sum, since K + S1 / n would round at the size of K, not of the mean.
//   adain     out = (x - mc) / sc * ss + ms on the statistics rounded to fp32, operation by operation.
//   epilogue  out_kind 0: v, fp32 NCHW; 1: u = min(max((v + 1) / 2, 0), 1), fp32 NCHW; 2: (uint8)(int)(u * 255.0f),
//             NHWC (the bytes Image.fromarray((255. * x).astype(np.uint8)) receives).  A NaN stays a NaN under kind 1,
//             as under torch's clamp, and becomes the byte 0.
//
// Kernels (no atomics, fixed orders, no capped grid: one workgroup per unit of work, 1-D grids):
//   colorfix_tile<DECOMP>  one workgroup of 1,024 threads per 64 x 64 output tile and plane.  With h_0 = 2^levels - 1
//                  and h_i = h_(i-1) - 2^(i-1) (31, 30, 28, 24, 16, 0 for five levels) the input is held at tile +- h_0
//                  and level i is formed at tile +- h_i only: rows pass A -> B on rows +- h_(i-1) x columns +- h_i,
//                  column pass B -> A on +- h_i both ways.  A clamped tap lies between the pixel and its unclamped tap,
//                  so inside the region the previous level wrote; positions of a region beyond the plane hold
//                  replicated values nobody inside the plane reads.  LDS: two fp32 [126][127] buffers = 128,016 B,
//                  dynamic (ONE workgroup of 16 waves per CU of 160 KiB).  Lanes run along a row in every pass: 32
//                  consecutive dwords per lane group, conflict-free; the stride 127 is odd.
//   colorfix_blur  one thread per element, nine clamped loads from global memory.
//   colorfix_partial, colorfix_fold   the statistics (two launches for one image or two).
//   colorfix_apply one thread per element.
#include <math.h>

#include "ssg_pixel.hpp"

namespace ssg {
namespace colorfix {

using pixel::NT;
using pixel::block_sum;
using pixel::check_workspace;

constexpr int T = 64;                       // output tile side
constexpr int MAXLEV = 5;
constexpr int HMAX = (1 << MAXLEV) - 1;     // 31: the halo of five levels
constexpr int RS = T + 2 * HMAX;            // 126: side of the haloed region
constexpr int LS = RS + 1;                  // 127: its row stride in LDS
constexpr int TILE_NT = 1024;
constexpr int CW = 128;                     // threads along a row of the region (>= RS), RG row groups of them
constexpr int RG = TILE_NT / CW;
static_assert(CW >= RS && (CW & (CW - 1)) == 0 && (T & (T - 1)) == 0, "the column masks");
constexpr int TILE_LDS = 2 * RS * LS * (int)sizeof(float);   // 128,016 B
constexpr int CHUNK = 4096;                 // elements per workgroup of colorfix_partial

struct TileArgs {
  const float *content;   // DECOMP: the image
  const float *style;
  void *out;              // fp32 NCHW or uint8 NHWC
  float *high, *low;      // DECOMP: either may be null
  int C, H, W, levels, out_kind, tiles_x, tiles_y;
};

__device__ __forceinline__ int clampi(int i, int n) { return min(max(i, 0), n - 1); }

// torch's clamp: a NaN stays a NaN (both comparisons are false)
__device__ __forceinline__ float unit(float v) {
  const float u = (v + 1.0f) / 2.0f;
  return u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u);
}

// element `at` of plane `p` (at = y W + x) under the three epilogues
__device__ __forceinline__ void store(void *out, int out_kind, float v, size_t p, size_t hw, size_t at, int C) {
  if (out_kind == SSG_COLORFIX_RAW) {
    ((float *)out)[p * hw + at] = v;
  } else if (out_kind == SSG_COLORFIX_UNIT) {
    ((float *)out)[p * hw + at] = unit(v);
  } else {
    const size_t n = p / C, c = p - n * C;
    ((uint8_t *)out)[(n * hw + at) * C + c] = (uint8_t)(int)(unit(v) * 255.0f);
  }
}

template <bool DECOMP>
__global__ __launch_bounds__(TILE_NT) void colorfix_tile(TileArgs a) {
  extern __shared__ __align__(16) float lds[];
  float *A = lds, *Bf = lds + RS * LS;
  const int tiles = a.tiles_x * a.tiles_y;
  const size_t plane = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - plane * tiles);
  const int ty0 = (tile / a.tiles_x) * T, tx0 = (tile % a.tiles_x) * T;
  const int H = a.H, W = a.W;
  const size_t hw = (size_t)H * W;
  const float *c = a.content + plane * hw;
  const float *s = DECOMP ? nullptr : a.style + plane * hw;
  const int h0 = (1 << a.levels) - 1;
  const int side0 = T + 2 * h0;           // local coordinate l <-> plane coordinate t0 - h0 + l
  const int oy = ty0 - h0, ox = tx0 - h0;

  // a thread keeps one column of the region and walks down its rows (no division; the clamped columns once per pass)
  const int col = threadIdx.x & (CW - 1), rg = threadIdx.x / CW;
  if (col < side0) {
    const int gx = clampi(ox + col, W);
    for (int ly = rg; ly < side0; ly += RG) {
      const size_t at = (size_t)clampi(oy + ly, H) * W + gx;
      A[ly * LS + col] = DECOMP ? c[at] : s[at] - c[at];
    }
  }
  __syncthreads();

  int hp = h0;                            // h_(i-1)
  for (int lev = 0; lev < a.levels; ++lev) {
    const int r = 1 << lev, hi = hp - r;
    const int lo_p = h0 - hp, n_p = T + 2 * hp;     // first local index and extent of region i-1
    const int lo_i = h0 - hi, n_i = T + 2 * hi;     // ... of region i
    const int lx = lo_i + col;
    // rows: A -> B on rows of region i-1, columns of region i
    if (col < n_i) {
      const int xm = clampi(ox + lx - r, W) - ox, xp = clampi(ox + lx + r, W) - ox;
      for (int ly = lo_p + rg; ly < lo_p + n_p; ly += RG) {
        const float *row = A + ly * LS;
        Bf[ly * LS + lx] = 0.25f * (row[xm] + row[xp]) + 0.5f * row[lx];
      }
    }
    __syncthreads();
    // columns: B -> A on region i
    if (col < n_i) {
      for (int ly = lo_i + rg; ly < lo_i + n_i; ly += RG) {
        const int gy = oy + ly;
        const int ym = clampi(gy - r, H) - oy, yp = clampi(gy + r, H) - oy;
        A[ly * LS + lx] = 0.25f * (Bf[ym * LS + lx] + Bf[yp * LS + lx]) + 0.5f * Bf[ly * LS + lx];
      }
    }
    __syncthreads();
    hp = hi;
  }

  {
    const int xx = threadIdx.x & (T - 1), x = tx0 + xx;
    for (int yy = threadIdx.x / T; yy < T; yy += TILE_NT / T) {
      const int y = ty0 + yy;
      if (y >= H || x >= W) break;
      const size_t at = (size_t)y * W + x;
      const float low = A[(h0 + yy) * LS + h0 + xx];
      if (DECOMP) {
        if (a.low) a.low[plane * hw + at] = low;
        if (a.high) a.high[plane * hw + at] = c[at] - low;
      } else {
        store(a.out, a.out_kind, c[at] + low, plane, hw, at, a.C);
      }
    }
  }
}

__global__ __launch_bounds__(NT) void colorfix_blur(const float *img, float *out, int H, int W, int radius, size_t n) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const size_t plane = i / hw, at = i - plane * hw;
  const int y = (int)(at / W), x = (int)(at - (size_t)y * W);
  // max(y - r, 0) and min(y + r, H - 1) without forming y + r (any radius >= 1 is legal)
  const int ys[3] = {y - min(radius, y), y, y + min(radius, H - 1 - y)};
  const int xm = x - min(radius, x), xp = x + min(radius, W - 1 - x);
  const float *p = img + plane * hw;
  float t[3];
  for (int k = 0; k < 3; ++k) {
    const float *row = p + (size_t)ys[k] * W;
    t[k] = 0.25f * (row[xm] + row[xp]) + 0.5f * row[x];
  }
  out[i] = 0.25f * (t[0] + t[2]) + 0.5f * t[1];
}

// ---- statistics ----
// part: (n_img, planes, nchunks, 3) fp64 {S0, S1, S2}, the last two about the plane's first element
__global__ __launch_bounds__(NT) void colorfix_partial(const float *x0, const float *x1, size_t hw, int nchunks,
                                                       size_t planes, double *part) {
  __shared__ double sh[NT / 64];
  const size_t unit_id = blockIdx.x;                      // (image, plane, chunk)
  const size_t pc = unit_id / nchunks;
  const int chunk = (int)(unit_id - pc * nchunks);
  const size_t im = pc / planes, plane = pc - im * planes;
  const float *p = (im ? x1 : x0) + plane * hw;
  const double K = (double)p[0];
  const size_t first = (size_t)chunk * CHUNK;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < CHUNK / NT; ++k) {
    const size_t at = first + (size_t)k * NT + threadIdx.x;
    if (at < hw) {
      const double v = (double)p[at], d = v - K;
      s0 += v;
      s1 += d;
      s2 += d * d;
    }
  }
  s0 = block_sum(s0, sh);
  __syncthreads();
  s1 = block_sum(s1, sh);
  __syncthreads();
  s2 = block_sum(s2, sh);
  if (threadIdx.x == 0) part[3 * unit_id] = s0, part[3 * unit_id + 1] = s1, part[3 * unit_id + 2] = s2;
}

// stats: (n_img, planes, 2) fp64 {mean, sqrt(var + eps)}
__global__ __launch_bounds__(NT) void colorfix_fold(size_t hw, int nchunks, const double *part, double eps,
                                                    double *stats) {
  __shared__ double sh[NT / 64];
  const size_t pc = blockIdx.x;                           // (image, plane)
  const double *q = part + 3 * pc * nchunks;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int k = threadIdx.x; k < nchunks; k += NT) s0 += q[3 * k], s1 += q[3 * k + 1], s2 += q[3 * k + 2];
  s0 = block_sum(s0, sh);
  __syncthreads();
  s1 = block_sum(s1, sh);
  __syncthreads();
  s2 = block_sum(s2, sh);
  if (threadIdx.x == 0) {
    const double n = (double)hw;
    stats[2 * pc] = s0 / n;
    stats[2 * pc + 1] = sqrt((s2 - s1 * s1 / n) / (n - 1.0) + eps);
  }
}

// stats null: the epilogue alone ('nofix')
__global__ __launch_bounds__(NT) void colorfix_apply(const float *x, const double *stats, size_t planes, size_t hw, int C,
                                                     int out_kind, void *out, size_t n) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const size_t plane = i / hw, at = i - plane * hw;
  float v = x[i];
  if (stats) {
    const float mc = (float)stats[2 * plane], sc = (float)stats[2 * plane + 1];
    const float ms = (float)stats[2 * (planes + plane)], ss = (float)stats[2 * (planes + plane) + 1];
    v = (v - mc) / sc * ss + ms;
  }
  store(out, out_kind, v, plane, hw, at, C);
}

// ---- host ----
inline int check_shape(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return SSG_E_BADARG;
  if ((double)B * C * H * W >= 2147483648.0) return SSG_E_TOOLARGE;
  return 0;
}

inline bool out_kind_ok(int k) { return k == SSG_COLORFIX_RAW || k == SSG_COLORFIX_UNIT || k == SSG_COLORFIX_U8_NHWC; }

inline int nchunks_of(int H, int W) { return (int)(((size_t)H * W + CHUNK - 1) / CHUNK); }

template <bool DECOMP>
inline int launch_tile(TileArgs &a, int B, hipStream_t st) {
  static std::atomic<unsigned long long> lds_set{0};
  if (const int rc = ensure_dynamic_lds(colorfix_tile<DECOMP>, TILE_LDS, lds_set)) return rc;
  a.tiles_x = (a.W + T - 1) / T, a.tiles_y = (a.H + T - 1) / T;
  // tiles x planes <= elements < 2^31
  const unsigned grid = (unsigned)((size_t)a.tiles_x * a.tiles_y * B * a.C);
  hipLaunchKernelGGL(colorfix_tile<DECOMP>, dim3(grid), dim3(TILE_NT), TILE_LDS, st, a);
  return (int)hipGetLastError();
}

}  // namespace colorfix
}  // namespace ssg

using namespace ssg::colorfix;

extern "C" {

int ssg_wavelet_blur(const float *image, int B, int C, int H, int W, int radius, float *out, ssg_stream_t stream) {
  if (!image || !out || image == out || radius < 1) return SSG_E_BADARG;
  if (const int rc = check_shape(B, C, H, W)) return rc;
  const size_t n = (size_t)B * C * H * W;
  hipLaunchKernelGGL(colorfix_blur, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, image, out, H,
                     W, radius, n);
  return (int)hipGetLastError();
}

int ssg_wavelet_decompose(const float *image, int B, int C, int H, int W, int levels, float *high, float *low,
                          ssg_stream_t stream) {
  if (!image || (!high && !low) || image == high || image == low || (high && high == low)) return SSG_E_BADARG;
  if (levels < 1) return SSG_E_BADARG;
  if (levels > MAXLEV) return SSG_E_TOOLARGE;
  if (const int rc = check_shape(B, C, H, W)) return rc;
  TileArgs a{};
  a.content = image, a.high = high, a.low = low;
  a.C = C, a.H = H, a.W = W, a.levels = levels;
  return launch_tile<true>(a, B, (hipStream_t)stream);
}

int ssg_colorfix_wavelet(const float *content, const float *style, int B, int C, int H, int W, int levels, int out_kind,
                         void *out, ssg_stream_t stream) {
  if (!content || !style || !out || out == (const void *)content || out == (const void *)style) return SSG_E_BADARG;
  if (levels < 1 || !out_kind_ok(out_kind)) return SSG_E_BADARG;
  if (levels > MAXLEV) return SSG_E_TOOLARGE;
  if (const int rc = check_shape(B, C, H, W)) return rc;
  TileArgs a{};
  a.content = content, a.style = style, a.out = out;
  a.C = C, a.H = H, a.W = W, a.levels = levels, a.out_kind = out_kind;
  return launch_tile<false>(a, B, (hipStream_t)stream);
}

size_t ssg_colorfix_workspace_bytes(int B, int C, int H, int W) {
  if (check_shape(B, C, H, W)) return 0;
  return ssg::align_up(sizeof(double) * 2 * 3 * (size_t)B * C * nchunks_of(H, W), 256);
}

int ssg_colorfix_stats(const float *content, const float *style, int B, int C, int H, int W, double eps, double *stats,
                       void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  if (!content || !stats || !workspace || !(eps >= 0.0)) return SSG_E_BADARG;
  if (const int rc = check_shape(B, C, H, W)) return rc;
  if (const int rc = check_workspace(workspace, workspace_bytes, ssg_colorfix_workspace_bytes(B, C, H, W))) return rc;
  const size_t planes = (size_t)B * C, hw = (size_t)H * W;
  const int nch = nchunks_of(H, W), n_img = style ? 2 : 1;
  if ((double)n_img * planes * nch >= 2147483648.0) return SSG_E_TOOLARGE;   // (planes of a few elements by the billion)
  double *part = (double *)workspace;
  hipLaunchKernelGGL(colorfix_partial, dim3((unsigned)(n_img * planes * nch)), dim3(NT), 0, (hipStream_t)stream, content,
                     style, hw, nch, planes, part);
  hipLaunchKernelGGL(colorfix_fold, dim3((unsigned)(n_img * planes)), dim3(NT), 0, (hipStream_t)stream, hw, nch,
                     (const double *)part, eps, stats);
  return (int)hipGetLastError();
}

int ssg_colorfix_adain(const float *content, const double *stats, int B, int C, int H, int W, int out_kind, void *out,
                       ssg_stream_t stream) {
  if (!content || !out || !out_kind_ok(out_kind)) return SSG_E_BADARG;
  if (out == (const void *)content && out_kind == SSG_COLORFIX_U8_NHWC) return SSG_E_BADARG;
  if (const int rc = check_shape(B, C, H, W)) return rc;
  const size_t planes = (size_t)B * C, hw = (size_t)H * W, n = planes * hw;
  hipLaunchKernelGGL(colorfix_apply, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, content, stats,
                     planes, hw, C, out_kind, out, n);
  return (int)hipGetLastError();
}

}  // extern "C"
