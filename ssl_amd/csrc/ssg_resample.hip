// Pillow's 8-bit convolution resize on the GPU: PIL.Image.resize(size, resample) with box=None and reducing_gap=None
// (ImagingResample, libImaging/Resample.c) for the five convolution filters -- what the Diffusion fork's load_img
// (test.py:111-120) and the two multiscale preparation scripts (generate_multiscale_img.py:27,42,
// generate_multiscale_DF2K.py:26,38) call with LANCZOS.  uint8 HWC in, C = 1 ('L') or 3 ('RGB'), a batch of same-size
// images, one launch per call.  The algorithm is integer from the tables on, so the result is Pillow's byte for byte.
//
// Contract:
//   tables    per axis with input size `in` and output size `out` (HOST, fp64, the C library's sin / cos as Pillow's C):
//             scale = in / out, fs = max(scale, 1), support = S fs, ksize = 2 ceil(support) + 1; for output index xx:
//             center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0),
//             n = min((int)(center + support + 0.5), in) - xmin, w_i = f((i + xmin - center + 0.5) (1 / fs)), i < n,
//             ww = their sum in index order, w_i /= ww when ww != 0; k_i = (int)(w_i 2^22 + 0.5) for w_i >= 0 and
//             (int)(w_i 2^22 - 0.5) otherwise; zeros from n to ksize.  bounds[xx] = {xmin, n}.
//   pass      clip8((2^21 + sum_i px[xmin + i] k_i) >> 22): int32 accumulator, arithmetic shift, clip to [0, 255].
//             Columns first into bytes, rows on those bytes; a pass whose axis keeps its size is not run.
//   epilogue  out_kind 0: the byte, HWC; 1: (float)v / 255.0f, fp32 NCHW; 2: 2.0f ((float)v / 255.0f) - 1.0f, fp32 NCHW
//             (compiled with -ffp-contract=off: load_img's numpy division and torch's multiply and subtract).
//
// Kernel (no atomics; image b of a batch gets the bytes it gets alone):
//   resample_tile  one workgroup of 256 threads per output tile and image, 1-D grid, no cap.  It stages the tile's
//                  coefficient rows and bounds (made relative to the footprint) as int32 in LDS, reads the input
//                  footprint -- rows ybounds[first].xmin .. ybounds[last].xmin + n, columns likewise -- into LDS with
//                  aligned dword loads (a row keeps its address's low two bits as a shift; words that straddle the
//                  ends of the tensor are read byte by byte), forms the column pass on every footprint row into a
//                  byte intermediate in LDS (lanes along the rows: the row pitches are 4 x odd, 32 lanes hit 32
//                  banks; the coefficient is one broadcast word) and the row pass from it (lanes along the bytes of an
//                  output row: consecutive bytes of the intermediate and of the output).
//   The tile comes from a short list: the first whose LDS is at most 20 KiB, else the one with the least LDS, which must
//   fit 160 KiB; the footprint of T outputs is at most ceil((T - 1) scale + 2 support) + 2 input pixels.  A table whose bounds leave that footprint (no table of
//   ssg_resample_table does) makes the workgroup return without writing.
#include <math.h>

#include <vector>

#include "ssg_pixel.hpp"

namespace ssg {
namespace resample {

using pixel::NT;

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int MAX_RATIO = 8;                 // in / out per axis the fused kernel takes
constexpr int LDS_LIMIT = 160 * 1024;
constexpr int LDS_PREF = 20 * 1024;
// (rows, columns), each divides the first; LANCZOS on three channels at 8 : 1 on both axes takes the last with 114,176 B,
// the most any supported call needs
constexpr int TILES[][2] = {{32, 64}, {16, 64}, {16, 32}, {8, 32}};
constexpr int N_TILES = (int)(sizeof(TILES) / sizeof(TILES[0]));

struct Args {
  const uint8_t *src;
  const uint8_t *src_end;
  void *out;
  const int *xb, *xk, *yb, *yk;   // null: that pass is not run
  int C, Hin, Win, Hout, Wout, kx, ky, out_kind;
  int TH, TW, tiles_x, tiles_y;
  int rows_max, cols_max;         // what the footprint may hold
  int pitchF, pitchM;             // bytes per footprint / intermediate row, 4 x odd
  int offF, offM;                 // byte offsets in LDS behind the int32 tables
};

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PRECISION_BITS, 0), 255); }

__device__ __forceinline__ void emit(const Args &a, size_t img, int y, int x, int c, int v) {
  if (a.out_kind == SSG_RESAMPLE_U8_HWC) {
    ((uint8_t *)a.out)[((img * a.Hout + y) * a.Wout + x) * a.C + c] = (uint8_t)v;
  } else {
    float f = (float)v / 255.0f;
    if (a.out_kind == SSG_RESAMPLE_F32_SIGNED) f = 2.0f * f - 1.0f;
    ((float *)a.out)[((img * a.C + c) * a.Hout + y) * a.Wout + x] = f;
  }
}

__global__ __launch_bounds__(NT) void resample_tile(Args a) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int tid = threadIdx.x;
  const int C = a.C, TH = a.TH, TW = a.TW;
  const bool HP = a.xb != nullptr, VP = a.yb != nullptr;
  int *kxs = (int *)lds;                        // [TW][kx]
  int *kys = kxs + TW * a.kx;                   // [TH][ky]
  int *bxs = kys + TH * a.ky;                   // [TW][2] {xmin - x0, n}
  int *bys = bxs + 2 * TW;                      // [TH][2]
  int &bad = bys[2 * TH];                       // a bound of the tile leaves its footprint
  unsigned char *F = lds + a.offF, *M = lds + a.offM;

  const int tiles = a.tiles_x * a.tiles_y;
  const size_t img = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - img * tiles);
  const int ty0 = (tile / a.tiles_x) * TH, tx0 = (tile % a.tiles_x) * TW;
  const int th = min(TH, a.Hout - ty0), tw = min(TW, a.Wout - tx0);

  // the footprint (the same words for every thread: the refusal below is uniform)
  int x0 = tx0, x1 = tx0 + tw, y0 = ty0, y1 = ty0 + th;
  if (HP) x0 = a.xb[2 * tx0], x1 = a.xb[2 * (tx0 + tw - 1)] + a.xb[2 * (tx0 + tw - 1) + 1];
  if (VP) y0 = a.yb[2 * ty0], y1 = a.yb[2 * (ty0 + th - 1)] + a.yb[2 * (ty0 + th - 1) + 1];
  if (x0 < 0 || x1 > a.Win || x1 <= x0 || x1 - x0 > a.cols_max) return;
  if (y0 < 0 || y1 > a.Hin || y1 <= y0 || y1 - y0 > a.rows_max) return;
  const int rows = y1 - y0, cols = x1 - x0;

  if (tid == 0) bad = 0;
  __syncthreads();
  if (HP) {
    for (int i = tid; i < tw * a.kx; i += NT) kxs[i] = a.xk[(size_t)tx0 * a.kx + i];
    for (int xx = tid; xx < tw; xx += NT) {
      const int b0 = a.xb[2 * (tx0 + xx)], n = a.xb[2 * (tx0 + xx) + 1];
      if (b0 < x0 || n < 0 || n > a.kx || b0 + n > x1) bad = 1;
      bxs[2 * xx] = b0 - x0, bxs[2 * xx + 1] = n;
    }
  }
  if (VP) {
    for (int i = tid; i < th * a.ky; i += NT) kys[i] = a.yk[(size_t)ty0 * a.ky + i];
    for (int yy = tid; yy < th; yy += NT) {
      const int b0 = a.yb[2 * (ty0 + yy)], n = a.yb[2 * (ty0 + yy) + 1];
      if (b0 < y0 || n < 0 || n > a.ky || b0 + n > y1) bad = 1;
      bys[2 * yy] = b0 - y0, bys[2 * yy + 1] = n;
    }
  }

  // footprint row r starts at byte g0 + r gs of the tensor; its aligned dwords go to F + r pitchF, so its first byte
  // sits at shift(r) = (address & 3) there
  const size_t gs = (size_t)a.Win * C;
  const uint8_t *g0 = a.src + ((img * a.Hin + y0) * a.Win + x0) * C;
  const unsigned lo = (unsigned)(uintptr_t)g0 & 3u, rs = (unsigned)(gs & 3u);
  const int nbytes = cols * C;
  const int ndw = (nbytes + 6) / 4;             // dwords of a row at the largest shift
  for (int item = tid; item < rows * ndw; item += NT) {
    const int r = item / ndw, d = item - r * ndw;
    const uint8_t *g = g0 + (size_t)r * gs;
    const unsigned sh = (unsigned)(uintptr_t)g & 3u;
    if (4 * d >= (int)sh + nbytes) continue;
    const uint8_t *p = g - sh + 4 * d;
    uint32_t w = 0;
    if (p >= a.src && p + 4 <= a.src_end) {
      w = *(const uint32_t *)p;
    } else {
      for (int j = 0; j < 4; ++j)
        if (p + j >= a.src && p + j < a.src_end) w |= (uint32_t)p[j] << (8 * j);
    }
    ((uint32_t *)(F + r * a.pitchF))[d] = w;
  }
  __syncthreads();
  if (bad) return;
  auto shift = [&](int r) { return (int)((lo + (unsigned)r * rs) & 3u); };

  const int Q = tw * C;                         // bytes of an output row of the tile
  if (HP) {
    for (int item = tid; item < rows * Q; item += NT) {
      int r, q;
      if (VP) q = item / rows, r = item - q * rows;     // lanes along the rows
      else r = item / Q, q = item - r * Q;              // no row pass follows: lanes along the stored bytes
      const int xx = q / C, c = q - xx * C;
      const int n = bxs[2 * xx + 1];
      const unsigned char *p = F + r * a.pitchF + shift(r) + bxs[2 * xx] * C + c;
      const int *k = kxs + xx * a.kx;
      int acc = 1 << (PRECISION_BITS - 1);
      for (int i = 0; i < n; ++i) acc += (int)p[i * C] * k[i];
      const int v = clip8(acc);
      if (VP) M[r * a.pitchM + q] = (unsigned char)v;
      else emit(a, img, ty0 + r, tx0 + xx, c, v);
    }
    if (!VP) return;
    __syncthreads();
  }
  for (int item = tid; item < th * Q; item += NT) {
    const int yy = item / Q, q = item - yy * Q;
    int v;
    if (VP) {
      const int b0 = bys[2 * yy], n = bys[2 * yy + 1];
      const int *k = kys + yy * a.ky;
      int acc = 1 << (PRECISION_BITS - 1);
      if (HP) {
        const unsigned char *p = M + b0 * a.pitchM + q;
        for (int i = 0; i < n; ++i) acc += (int)p[i * a.pitchM] * k[i];
      } else {
        for (int i = 0; i < n; ++i) acc += (int)F[(b0 + i) * a.pitchF + shift(b0 + i) + q] * k[i];
      }
      v = clip8(acc);
    } else {
      v = F[yy * a.pitchF + shift(yy) + q];
    }
    const int xx = q / C;
    emit(a, img, ty0 + yy, tx0 + xx, q - xx * C, v);
  }
}

// ---------------------------------------------------------------------------------------------------------- host ---
// Pillow's filters (Resample.c), fp64 on the C library's sin / cos
inline double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

inline double filter_value(int filter, double x) {
  switch (filter) {
    case SSG_RESAMPLE_LANCZOS:
      return (-3.0 <= x && x < 3.0) ? sinc_filter(x) * sinc_filter(x / 3) : 0.0;
    case SSG_RESAMPLE_BILINEAR:
      if (x < 0.0) x = -x;
      return x < 1.0 ? 1.0 - x : 0.0;
    case SSG_RESAMPLE_BICUBIC: {
      const double a = -0.5;
      if (x < 0.0) x = -x;
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
      if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
      return 0.0;
    }
    case SSG_RESAMPLE_BOX:
      return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    default:   // SSG_RESAMPLE_HAMMING
      if (x < 0.0) x = -x;
      if (x == 0.0) return 1.0;
      if (x >= 1.0) return 0.0;
      x = x * M_PI;
      return sin(x) / x * (0.54f + 0.46f * cos(x));
  }
}

inline double filter_support(int filter) {
  switch (filter) {
    case SSG_RESAMPLE_LANCZOS: return 3.0;
    case SSG_RESAMPLE_BICUBIC: return 2.0;
    case SSG_RESAMPLE_BOX: return 0.5;
    default: return 1.0;   // BILINEAR, HAMMING
  }
}

inline bool filter_ok(int f) { return f >= SSG_RESAMPLE_LANCZOS && f <= SSG_RESAMPLE_HAMMING; }

// the most input pixels under t consecutive outputs of an axis
inline int footprint(int t, int in, int out, int filter) {
  const double scale = (double)in / out, support = filter_support(filter) * (scale < 1.0 ? 1.0 : scale);
  const double span = ceil((t - 1) * scale + 2.0 * support) + 2.0;
  return span < (double)in ? (int)span : in;
}

inline int odd_dwords(int bytes) { return 4 * (((bytes + 3) / 4) | 1); }

// fills the tile geometry of `a` (C, the sizes and the tables already set): the first tile of the list whose LDS is at
// most LDS_PREF (eight workgroups, 32 waves, per CU), else the tile with the least LDS; false: none fits.  Measured on
// the four multiscale resizes of a 2040 x 1356 RGB image: taking the first tile that fits 160 KiB instead costs 3.6 x
// on the 1 / 3 scale (one workgroup of four waves per CU), DESIGN section 19.
inline bool choose_tile(Args &a, int filter, size_t *lds_bytes) {
  const bool HP = a.xb != nullptr, VP = a.yb != nullptr;
  const size_t pref = (size_t)env_int("SSG_RESAMPLE_LDS_PREF", LDS_PREF);   // (the profiling build's A/B switch)
  size_t best = (size_t)LDS_LIMIT + 1;
  for (int t = 0; t < N_TILES; ++t) {
    const int TH = TILES[t][0], TW = TILES[t][1];
    const int cols = HP ? footprint(TW, a.Win, a.Wout, filter) : TW;
    const int rows = VP ? footprint(TH, a.Hin, a.Hout, filter) : TH;
    const int pitchF = odd_dwords(cols * a.C + 6), pitchM = (HP && VP) ? odd_dwords(TW * a.C) : 0;
    const size_t ints = sizeof(int) * ((size_t)TW * a.kx + (size_t)TH * a.ky + 2 * TW + 2 * TH + 4);
    const size_t total = ints + (size_t)rows * pitchF + (size_t)rows * pitchM;
    if (total >= best) continue;
    best = total;
    a.TH = TH, a.TW = TW, a.rows_max = rows, a.cols_max = cols, a.pitchF = pitchF, a.pitchM = pitchM;
    a.offF = (int)ints, a.offM = (int)(ints + (size_t)rows * pitchF);
    *lds_bytes = total;
    if (total <= pref) break;
  }
  return best <= (size_t)LDS_LIMIT;
}

}  // namespace resample

static int resample_max_ratio() { return resample::MAX_RATIO; }

static void resample_tile_shape(int *th, int *tw) { *th = resample::TILES[0][0], *tw = resample::TILES[0][1]; }

static int resample_ksize(int in, int out, int filter) {
  if (in < 1 || out < 1 || !resample::filter_ok(filter)) return SSG_E_BADARG;
  double fs = (double)in / out;
  if (fs < 1.0) fs = 1.0;
  const double c = ceil(resample::filter_support(filter) * fs);
  if (c > 1073741000.0) return SSG_E_TOOLARGE;
  return (int)c * 2 + 1;
}

static int resample_table(int in, int out, int filter, int *bounds, int *coef) {
  using namespace resample;
  if (!bounds || !coef) return SSG_E_BADARG;
  const int ksize = resample_ksize(in, out, filter);
  if (ksize < 0) return ksize;
  const double scale = (double)in / out;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filter_support(filter) * filterscale, ss = 1.0 / filterscale;
  std::vector<double> w((size_t)ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += w[x] = filter_value(filter, (x + xmin - center + 0.5) * ss);
    int *k = coef + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      double v = x < xmax ? w[x] : 0.0;
      if (x < xmax && ww != 0.0) v /= ww;
      k[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
    }
    bounds[2 * xx] = xmin, bounds[2 * xx + 1] = xmax;
  }
  return 0;
}

static int launch_resample(const uint8_t *src, int B, int C, int Hin, int Win, int Hout, int Wout, int filter,
                           const int *xbounds, const int *xcoef, const int *ybounds, const int *ycoef, int out_kind, void *out,
                           hipStream_t st) {
  using namespace resample;
  if (!src || !out || (const void *)src == out) return SSG_E_BADARG;
  if (B < 1 || (C != 1 && C != 3) || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || !filter_ok(filter)) return SSG_E_BADARG;
  if (out_kind != SSG_RESAMPLE_U8_HWC && out_kind != SSG_RESAMPLE_F32_UNIT && out_kind != SSG_RESAMPLE_F32_SIGNED)
    return SSG_E_BADARG;
  const bool HP = Win != Wout, VP = Hin != Hout;
  if ((HP && (!xbounds || !xcoef)) || (VP && (!ybounds || !ycoef))) return SSG_E_BADARG;
  if ((double)B * C * Hin * Win >= 2147483648.0 || (double)B * C * Hout * Wout >= 2147483648.0) return SSG_E_TOOLARGE;
  if ((long long)Win > (long long)MAX_RATIO * Wout || (long long)Hin > (long long)MAX_RATIO * Hout) return SSG_E_TOOLARGE;
  Args a{};
  a.src = src, a.src_end = src + (size_t)B * Hin * Win * C, a.out = out;
  a.xb = HP ? xbounds : nullptr, a.xk = HP ? xcoef : nullptr, a.yb = VP ? ybounds : nullptr, a.yk = VP ? ycoef : nullptr;
  a.C = C, a.Hin = Hin, a.Win = Win, a.Hout = Hout, a.Wout = Wout, a.out_kind = out_kind;
  a.kx = HP ? resample_ksize(Win, Wout, filter) : 0, a.ky = VP ? resample_ksize(Hin, Hout, filter) : 0;
  size_t lds_bytes = 0;
  if (!choose_tile(a, filter, &lds_bytes)) return SSG_E_TOOLARGE;
  a.tiles_x = (Wout + a.TW - 1) / a.TW, a.tiles_y = (Hout + a.TH - 1) / a.TH;
  static std::atomic<unsigned long long> lds_set{0};
  if (const int rc = ensure_dynamic_lds(resample_tile, LDS_LIMIT, lds_set)) return rc;
  // tiles x images <= output pixels < 2^31
  const unsigned grid = (unsigned)((size_t)a.tiles_x * a.tiles_y * B);
  hipLaunchKernelGGL(resample::resample_tile, dim3(grid), dim3(NT), lds_bytes, st, a);
  return (int)hipGetLastError();
}

}  // namespace ssg

extern "C" {

int ssg_resample_ksize(int in, int out, int filter) { return ssg::resample_ksize(in, out, filter); }

int ssg_resample_table(int in, int out, int filter, int *bounds, int *coef) {
  return ssg::resample_table(in, out, filter, bounds, coef);
}

int ssg_resample_tile(int *th, int *tw) {
  if (!th || !tw) return SSG_E_BADARG;
  ssg::resample_tile_shape(th, tw);
  return 0;
}

int ssg_resample_max_ratio(void) { return ssg::resample_max_ratio(); }

int ssg_resample(const uint8_t *src, int B, int C, int Hin, int Win, int Hout, int Wout, int filter, const int *xbounds,
                 const int *xcoef, const int *ybounds, const int *ycoef, int out_kind, void *out, ssg_stream_t stream) {
  return ssg::launch_resample(src, B, C, Hin, Win, Hout, Wout, filter, xbounds, xcoef, ybounds, ycoef, out_kind, out,
                              (hipStream_t)stream);
}

}  // extern "C"
