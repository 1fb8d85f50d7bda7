// MATLAB's bicubic imresize as the reference restates it in Python (basicsr/utils/matlab_functions.py:imresize, KAIR's
// utils_image.py:imresize / imresize_np; the .m script generate_bicubic_img.m calls the original): any positive scale,
// up or down, with or without antialiasing, output sides ceil(n scale), one weight row per output pixel, symmetric
// mirror at the borders.  Evaluated in fp64 (MATLAB forms its coordinates in doubles; the reference's Python forms them
// in float32 and drifts with the image side), one launch per call for a batch of planes.
//
// Contract (per axis: input length n, scale s > 0, both passes use the same s):
//   m      = ceil(n s), in doubles on the host.
//   taps   kw = 4 / s when s < 1 and antialiasing is on, else 4; T = ceil(kw) taps per output.
//   table  for output k = 1 .. m (1-based): u = k / s + 0.5 (1 - 1 / s), left = floor(u - kw / 2), taps j = left + 1 ..
//          left + T, v_j = s c(s (u - j)) under antialiasing and c(u - j) otherwise, with Keys' cubic
//          c(x) = (1.5 |x|^3 - 2.5 |x|^2) + 1 for |x| <= 1, ((-0.5 |x|^3 + 2.5 |x|^2) - 4 |x|) + 2 for |x| <= 2, else 0,
//          |x|^2 = |x| |x| and |x|^3 = |x|^2 |x|; w_j = v_j / V with V the sum of the v_j in index order from 0.0.  All
//          fp64, every operation rounded on its own (-ffp-contract=off), so the host function and the restatement in
//          tests/imresize_reference.py agree bit for bit.  first[k - 1] = left is the first tap's 0-BASED index.
//   mirror 0-based tap j < 0 reads -1 - j, j >= n reads 2 n - 1 - j (symmetric, the border sample repeated): applied
//          to the index, once.  Every tap of every output must lie in [-n, 2 n - 1]; an axis that leaves it is refused
//          (SSG_E_IMAGESMALL) on the host, from first[0] and first[m - 1].
//   passes COLUMNS first (each output column of every input row), then ROWS: t[r][x] = sum_i wx[x][i] src[r][fx[x] + i],
//          y[q][x] = sum_i wy[q][i] t[fy[q] + i][x], fp64 sums in tap order from 0.0, products rounded before the add.
//          (The reference filters the rows first; in exact arithmetic the two orders agree.)
//   out    SSG_IMRESIZE_F32_PLANES (float)y, rounded once; SSG_IMRESIZE_U8_HWC min(255, floor(y + 0.5)) for y >= 0 and
//          0 below (MATLAB's round-half-away on uint8; y is the sum over the byte values 0 .. 255 themselves);
//          SSG_IMRESIZE_F32_UNIT (float)that byte / 255.0f, fp32 (B,C,h,w).
//
// Kernel (no atomics; plane b of a batch gets the bits it gets alone):
//   imresize_tile  one workgroup of 256 threads per output tile and plane, 1-D grid, no cap.  LDS, in this order:
//                  the tile's weight rows as doubles, the fp64 intermediate, the first indices made relative to the
//                  footprint, the footprint as fp32 (a byte is exact in it).  The footprint -- rows first[ty0] ..
//                  first[ty0 + th - 1] + Ty, columns likewise -- is read with the mirror applied to the index, lanes
//                  along a row.  Column pass LDS -> LDS: lanes along the footprint ROWS of one output column (the
//                  footprint's pitch is an odd number of dwords, so the 32 lanes of a half-wave -- the unit within which
//                  LDS accesses conflict -- read 32 different banks; the intermediate's pitch is an odd number of
//                  doubles, so their fp64 stores fall evenly on the banks, two dwords each, the two cycles such a store
//                  takes at best; the weight and the first index are one broadcast word).  Row pass LDS -> registers -> global: lanes along the columns of one
//                  output row, consecutive doubles of the intermediate and consecutive outputs.
//   The tile comes from a short list: the first whose LDS is at most 48 KiB (three workgroups a CU), else the one with
//   the least LDS, which must fit 160 KiB; t outputs of an axis cover at most ceil((t - 1) / s) + T + 1 input pixels.
//   Where that span exceeds t T (a steep scale without antialiasing: the taps of neighbouring outputs do not touch) the
//   footprint of the axis is COMPACT instead, T entries per output, so that every non-antialiased scale fits.
//   A table whose indices leave that footprint or the mirror domain (none of ssg_imresize_table does) makes the
//   workgroup return without writing; every load is clamped into the plane besides.
#include <math.h>

#include "ssg_pixel.hpp"

namespace ssg {
namespace imresize {

using pixel::NT;

constexpr int MAX_TAPS = 32;
constexpr int LDS_LIMIT = 160 * 1024;
constexpr int LDS_PREF = 48 * 1024;
// (rows, columns).  32 x 64 serves every upscale (a footprint of a few pixels); antialiased 1 / 2 takes 16 x 32, 1 / 4
// takes 8 x 32 with 42,548 B and 1 / 8 takes 8 x 16 with 72,820 B, the most any call needs (a compact footprint is at
// most 4 t entries an axis).  Timed at 1 / 4 (profiles/imresize_tile_ab.txt): 8 x 16, 8 x 32 and
// 16 x 32 lie within 20 % of each other and no tile wins both shapes, so the preference stays where LDS bytes put it.
constexpr int TILES[][2] = {{32, 64}, {16, 32}, {8, 32}, {8, 16}};
constexpr int N_TILES = (int)(sizeof(TILES) / sizeof(TILES[0]));

struct Args {
  const void *src;
  void *out;
  const int *xf, *yf;             // first 0-based tap per output column / row (before the mirror)
  const double *xw, *yw;          // [Wout][Tx], [Hout][Ty]
  int in_kind, out_kind, C, Hin, Win, Hout, Wout, Tx, Ty;
  int TH, TW, tiles_x, tiles_y;
  int rows_max, cols_max;         // what the footprint may hold
  int cx, cy;                     // the footprint of that axis is compact: T entries per output, no sharing
  int pitchF, pitchM;             // floats per footprint row, doubles per intermediate row, both odd
  int offM, offI, offF;           // byte offsets in LDS behind the weight rows
};

// symmetric mirror of a 0-based index, one reflection; the clamp keeps a foreign table's loads inside the plane
__device__ __forceinline__ int mirror(int j, int n) {
  j = j < 0 ? -1 - j : j;
  j = j >= n ? 2 * n - 1 - j : j;
  return min(max(j, 0), n - 1);
}

__device__ __forceinline__ void emit(const Args &a, int plane, int y, int x, double acc) {
  if (a.out_kind == SSG_IMRESIZE_F32_PLANES) {
    ((float *)a.out)[((size_t)plane * a.Hout + y) * a.Wout + x] = (float)acc;
    return;
  }
  const double r = floor(acc + 0.5);
  const int v = acc >= 0.0 ? (r > 255.0 ? 255 : (int)r) : 0;
  if (a.out_kind == SSG_IMRESIZE_U8_HWC) {
    const int b = plane / a.C, c = plane - b * a.C;
    ((uint8_t *)a.out)[(((size_t)b * a.Hout + y) * a.Wout + x) * a.C + c] = (uint8_t)v;
  } else {
    ((float *)a.out)[((size_t)plane * a.Hout + y) * a.Wout + x] = (float)v / 255.0f;
  }
}

__global__ __launch_bounds__(NT) void imresize_tile(Args a) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int tid = threadIdx.x;
  const int TH = a.TH, TW = a.TW, Tx = a.Tx, Ty = a.Ty;
  double *wxs = (double *)lds;                  // [TW][Tx]
  double *wys = wxs + TW * Tx;                  // [TH][Ty]
  double *M = (double *)(lds + a.offM);         // [rows][pitchM]
  int *bxs = (int *)(lds + a.offI);             // [TW] first column - x0
  int *bys = bxs + TW;                          // [TH] first row - y0
  int &bad = bys[TH];                           // an index of the tile leaves its footprint
  float *F = (float *)(lds + a.offF);           // [rows][pitchF]

  const int tiles = a.tiles_x * a.tiles_y;
  const int plane = blockIdx.x / tiles;
  const int tile = blockIdx.x - plane * tiles;
  const int ty0 = (tile / a.tiles_x) * TH, tx0 = (tile % a.tiles_x) * TW;
  const int th = min(TH, a.Hout - ty0), tw = min(TW, a.Wout - tx0);

  // the footprint, before the mirror (the same words for every thread: the refusal below is uniform).  Contiguous:
  // the span of the tile's taps.  Compact (the taps of neighbouring outputs lie further apart than they are wide, a
  // steep scale without antialiasing): T entries per output, entry xx T + i holds tap i of output xx.
  const int x0 = a.cx ? 0 : a.xf[tx0], x1 = a.cx ? tw * Tx : a.xf[tx0 + tw - 1] + Tx;
  const int y0 = a.cy ? 0 : a.yf[ty0], y1 = a.cy ? th * Ty : a.yf[ty0 + th - 1] + Ty;
  if (x1 - x0 < Tx || x1 - x0 > a.cols_max || y1 - y0 < Ty || y1 - y0 > a.rows_max) return;
  const int rows = y1 - y0, cols = x1 - x0;

  if (tid == 0) bad = 0;
  __syncthreads();
  for (int i = tid; i < tw * Tx; i += NT) wxs[i] = a.xw[(size_t)tx0 * Tx + i];
  for (int i = tid; i < th * Ty; i += NT) wys[i] = a.yw[(size_t)ty0 * Ty + i];
  for (int xx = tid; xx < tw; xx += NT) {
    const int b0 = a.xf[tx0 + xx];
    if (b0 < -a.Win || b0 + Tx > 2 * a.Win || (!a.cx && (b0 < x0 || b0 + Tx > x1))) bad = 1;
    bxs[xx] = a.cx ? xx * Tx : b0 - x0;
  }
  for (int yy = tid; yy < th; yy += NT) {
    const int b0 = a.yf[ty0 + yy];
    if (b0 < -a.Hin || b0 + Ty > 2 * a.Hin || (!a.cy && (b0 < y0 || b0 + Ty > y1))) bad = 1;
    bys[yy] = a.cy ? yy * Ty : b0 - y0;
  }

  const int img = plane / a.C, ch = plane - img * a.C;
  for (int item = tid; item < rows * cols; item += NT) {
    const int r = item / cols, c = item - r * cols;
    const int gy = a.cy ? a.yf[ty0 + r / Ty] + r % Ty : y0 + r, gx = a.cx ? a.xf[tx0 + c / Tx] + c % Tx : x0 + c;
    const size_t sy = (size_t)mirror(gy, a.Hin), sx = (size_t)mirror(gx, a.Win);
    float v;
    if (a.in_kind == SSG_IMRESIZE_IN_F32) v = ((const float *)a.src)[((size_t)plane * a.Hin + sy) * a.Win + sx];
    else v = (float)((const uint8_t *)a.src)[(((size_t)img * a.Hin + sy) * a.Win + sx) * a.C + ch];
    F[r * a.pitchF + c] = v;
  }
  __syncthreads();
  if (bad) return;

  // columns: lanes along the footprint rows of one output column
  for (int item = tid; item < rows * tw; item += NT) {
    const int xx = item / rows, r = item - xx * rows;
    const float *p = F + r * a.pitchF + bxs[xx];
    const double *w = wxs + xx * Tx;
    double acc = 0.0;
    for (int i = 0; i < Tx; ++i) acc += w[i] * (double)p[i];
    M[r * a.pitchM + xx] = acc;
  }
  __syncthreads();
  // rows: lanes along the columns of one output row
  for (int item = tid; item < th * tw; item += NT) {
    const int yy = item / tw, xx = item - yy * tw;
    const double *p = M + bys[yy] * a.pitchM + xx;
    const double *w = wys + yy * Ty;
    double acc = 0.0;
    for (int i = 0; i < Ty; ++i) acc += w[i] * p[i * a.pitchM];
    emit(a, plane, ty0 + yy, tx0 + xx, acc);
  }
}

// ---------------------------------------------------------------------------------------------------------- host ---
inline double cubic(double x) {
  const double ax = fabs(x), ax2 = ax * ax, ax3 = ax2 * ax;
  if (ax <= 1.0) return (1.5 * ax3 - 2.5 * ax2) + 1.0;
  if (ax <= 2.0) return ((-0.5 * ax3 + 2.5 * ax2) - 4.0 * ax) + 2.0;
  return 0.0;
}

inline bool scale_ok(double s) { return s > 0.0 && s <= 1.7976931348623157e308; }   // (false for a NaN)

inline double coordinate(int k, double s) { return k / s + 0.5 * (1.0 - 1.0 / s); }

// left of output k (1-based) as a double: floor(u - kw / 2)
inline double left_of(int k, double s, double kw) { return floor(coordinate(k, s) - kw / 2.0); }

// the mirror domain of an axis, from its first and its last output (left never decreases with k)
inline bool axis_in_domain(int n, int m, double s, double kw, int T) {
  return left_of(1, s, kw) >= -(double)n && left_of(m, s, kw) + T <= 2.0 * n;
}

// the most input pixels under t consecutive outputs of an axis: left moves by at most ceil((t - 1) / s) over them when
// u is exact, and by one more when a rounding of u crosses an integer
inline double footprint(int t, double s, int T) { return ceil((t - 1) / s) + T + 1; }

// fills the tile geometry of `a` for tile t of the list and returns its LDS bytes
inline size_t tile_geometry(Args &a, int t, double s) {
  const int TH = TILES[t][0], TW = TILES[t][1];
  double rows = footprint(TH, s, a.Ty), cols = footprint(TW, s, a.Tx);
  a.cy = rows > (double)TH * a.Ty, a.cx = cols > (double)TW * a.Tx;
  if (a.cy) rows = (double)TH * a.Ty;
  if (a.cx) cols = (double)TW * a.Tx;
  const int pitchF = (int)cols | 1, pitchM = TW | 1;
  const size_t wbytes = sizeof(double) * ((size_t)TW * a.Tx + (size_t)TH * a.Ty);
  const size_t mbytes = sizeof(double) * (size_t)rows * pitchM;
  const size_t ibytes = sizeof(int) * (size_t)((TW + TH + 2) & ~1);
  a.TH = TH, a.TW = TW, a.rows_max = (int)rows, a.cols_max = (int)cols, a.pitchF = pitchF, a.pitchM = pitchM;
  a.offM = (int)wbytes, a.offI = (int)(wbytes + mbytes), a.offF = (int)(wbytes + mbytes + ibytes);
  return wbytes + mbytes + ibytes + sizeof(float) * (size_t)rows * pitchF;
}

// the first tile of the list whose LDS is at most LDS_PREF, else the tile with the least LDS; -1: none fits 160 KiB
inline int choose_tile(Args &a, double s, size_t *lds_bytes) {
  const size_t pref = (size_t)env_int("SSG_IMRESIZE_LDS_PREF", LDS_PREF);   // (the profiling build's A/B switch)
  size_t best = (size_t)LDS_LIMIT + 1;
  int which = -1;
  for (int t = 0; t < N_TILES; ++t) {
    Args g = a;
    const size_t total = tile_geometry(g, t, s);
    if (total >= best) continue;
    best = total, which = t;
    if (total <= pref) break;
  }
  if (which >= 0) *lds_bytes = tile_geometry(a, which, s);
  return which;
}

}  // namespace imresize

static int imresize_out_size(int n, double scale) {
  if (n < 1 || !imresize::scale_ok(scale)) return SSG_E_BADARG;
  const double m = ceil((double)n * scale);
  if (m < 1.0) return SSG_E_BADARG;
  if (m >= 2147483648.0) return SSG_E_TOOLARGE;
  return (int)m;
}

static int imresize_taps(double scale, int antialias) {
  if (!imresize::scale_ok(scale)) return SSG_E_BADARG;
  const double kw = (scale < 1.0 && antialias) ? 4.0 / scale : 4.0;
  const double t = ceil(kw);
  return t > imresize::MAX_TAPS ? SSG_E_TOOLARGE : (int)t;
}

// the checks of one axis that every entry point shares: the size, the taps and the mirror domain
static int imresize_axis(int n, int m, double scale, int antialias, double *kw_out, int *taps_out) {
  const int want = imresize_out_size(n, scale);
  if (want < 0) return want;
  if (m != want) return SSG_E_BADARG;
  const int T = imresize_taps(scale, antialias);
  if (T < 0) return T;
  const double kw = (scale < 1.0 && antialias) ? 4.0 / scale : 4.0;
  if (!imresize::axis_in_domain(n, m, scale, kw, T)) return SSG_E_IMAGESMALL;
  *kw_out = kw, *taps_out = T;
  return 0;
}

static int imresize_table(int n, int m, double scale, int antialias, int *first, double *weights) {
  using namespace imresize;
  if (!first || !weights) return SSG_E_BADARG;
  double kw = 0.0;
  int T = 0;
  if (const int rc = imresize_axis(n, m, scale, antialias, &kw, &T)) return rc;
  const bool aa = scale < 1.0 && antialias;
  for (int k = 1; k <= m; ++k) {
    const double u = coordinate(k, scale), left = floor(u - kw / 2.0);
    double *w = weights + (size_t)(k - 1) * T;
    double sum = 0.0;
    for (int i = 0; i < T; ++i) {
      const double d = u - (left + 1.0 + i);
      w[i] = aa ? scale * cubic(scale * d) : cubic(d);
      sum += w[i];
    }
    for (int i = 0; i < T; ++i) w[i] /= sum;
    first[k - 1] = (int)left;                   // the 0-based index of the 1-based tap left + 1
  }
  return 0;
}

static int imresize_tiles(double scale, int antialias, int *tiles, int capacity, int *chosen) {
  using namespace imresize;
  if (capacity < 0 || (capacity > 0 && !tiles)) return SSG_E_BADARG;
  for (int t = 0; t < N_TILES && t < capacity; ++t) tiles[2 * t] = TILES[t][0], tiles[2 * t + 1] = TILES[t][1];
  if (chosen) {
    *chosen = -1;
    const int T = imresize_taps(scale, antialias);
    if (T > 0) {
      Args a{};
      a.Tx = a.Ty = T;
      size_t lds_bytes = 0;
      *chosen = choose_tile(a, scale, &lds_bytes);
    }
  }
  return N_TILES;
}

static int launch_imresize(const void *src, int in_kind, int B, int C, int Hin, int Win, double scale, int antialias,
                           const int *yfirst, const double *yweights, const int *xfirst, const double *xweights, int out_kind,
                           void *out, hipStream_t st) {
  using namespace imresize;
  if (!src || !out || src == out || !yfirst || !yweights || !xfirst || !xweights) return SSG_E_BADARG;
  if (B < 1 || C < 1 || Hin < 1 || Win < 1) return SSG_E_BADARG;
  if (in_kind == SSG_IMRESIZE_IN_F32) {
    if (out_kind != SSG_IMRESIZE_F32_PLANES) return SSG_E_BADARG;
  } else if (in_kind == SSG_IMRESIZE_IN_U8_HWC) {
    if (C != 1 && C != 3) return SSG_E_BADARG;
    if (out_kind != SSG_IMRESIZE_U8_HWC && out_kind != SSG_IMRESIZE_F32_UNIT) return SSG_E_BADARG;
  } else {
    return SSG_E_BADARG;
  }
  if (!scale_ok(scale)) return SSG_E_BADARG;
  const int Hout = imresize_out_size(Hin, scale), Wout = imresize_out_size(Win, scale);
  if (Hout < 0) return Hout;
  if (Wout < 0) return Wout;
  if ((double)B * C * Hin * Win >= 2147483648.0 || (double)B * C * Hout * Wout >= 2147483648.0) return SSG_E_TOOLARGE;
  double kw = 0.0;
  int T = 0;
  if (const int rc = imresize_axis(Hin, Hout, scale, antialias, &kw, &T)) return rc;
  if (const int rc = imresize_axis(Win, Wout, scale, antialias, &kw, &T)) return rc;
  Args a{};
  a.src = src, a.out = out, a.xf = xfirst, a.yf = yfirst, a.xw = xweights, a.yw = yweights;
  a.in_kind = in_kind, a.out_kind = out_kind, a.C = C, a.Hin = Hin, a.Win = Win, a.Hout = Hout, a.Wout = Wout;
  a.Tx = a.Ty = T;
  size_t lds_bytes = 0;
  if (choose_tile(a, scale, &lds_bytes) < 0) return SSG_E_TOOLARGE;
  a.tiles_x = (Wout + a.TW - 1) / a.TW, a.tiles_y = (Hout + a.TH - 1) / a.TH;
  static std::atomic<unsigned long long> lds_set{0};
  if (const int rc = ensure_dynamic_lds(imresize_tile, LDS_LIMIT, lds_set)) return rc;
  // tiles x planes <= output elements < 2^31
  const unsigned grid = (unsigned)((size_t)a.tiles_x * a.tiles_y * B * C);
  hipLaunchKernelGGL(imresize::imresize_tile, dim3(grid), dim3(NT), lds_bytes, st, a);
  return (int)hipGetLastError();
}

}  // namespace ssg

extern "C" {

int ssg_imresize_out_size(int n, double scale) { return ssg::imresize_out_size(n, scale); }

int ssg_imresize_taps(double scale, int antialias) { return ssg::imresize_taps(scale, antialias); }

int ssg_imresize_table(int n, int m, double scale, int antialias, int *first, double *weights) {
  return ssg::imresize_table(n, m, scale, antialias, first, weights);
}

int ssg_imresize_tiles(double scale, int antialias, int *tiles, int capacity, int *chosen) {
  return ssg::imresize_tiles(scale, antialias, tiles, capacity, chosen);
}

int ssg_imresize(const void *src, int in_kind, int B, int C, int Hin, int Win, double scale, int antialias,
                 const int *yfirst, const double *yweights, const int *xfirst, const double *xweights, int out_kind,
                 void *out, ssg_stream_t stream) {
  return ssg::launch_imresize(src, in_kind, B, C, Hin, Win, scale, antialias, yfirst, yweights, xfirst, xweights,
                              out_kind, out, (hipStream_t)stream);
}

}  // extern "C"
