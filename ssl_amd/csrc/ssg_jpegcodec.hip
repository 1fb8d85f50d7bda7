// libjpeg's baseline JPEG round trip -- encode at a quality, decode again -- without the bitstream: what the reference
// reaches through cv2.imencode / cv2.imdecode (KAIR's add_JPEG_noise, basicsr's add_jpg_compression, util_image's
// jpeg_compress).  Entropy coding is lossless, so the decoded pixels are fixed by eight integer stages, restated in
// tests/jpeg_codec_reference.py, which this file is held to bit for bit: colour conversion, 2 x 2 chroma downsampling,
// the "islow" forward DCT, quantisation, dequantisation, the "islow" inverse DCT, fancy chroma upsampling and the
// colour conversion back (jpeg_set_quality(q, force_baseline), 4:2:0, JDCT_ISLOW, fancy upsampling, no smoothing).
//
// Contract (every shift arithmetic, every value int32: |a DCT intermediate| < 2^31 for 8-bit samples):
//   in      SSG_JPEG_IN_U8_HWC uint8 (B,H,W,C); SSG_JPEG_IN_F32_NCHW fp32 (B,C,H,W), v = rint(min(max(x, 0), 1) 255.0f).
//   colour  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,
//           Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16.  C = 1: Y is the byte.
//   edges   a Y sample outside the image is the pixel at (min(y, H - 1), min(x, W - 1)).  Chroma sample (r, c) of the
//           downsampled plane, r' = min(r, ceil(H / 2) - 1): (sum of Cb over rows min(2 r', H - 1), min(2 r' + 1, H - 1)
//           and columns min(2 c, W - 1), min(2 c + 1, W - 1), + 1 for even c, + 2 for odd c) >> 2: the full-resolution
//           plane is replicated to the right and by at most one row, the DOWNSAMPLED rows fill the MCU row.
//   blocks  8 x 8: samples - 128, forward rows then columns; q = sign(c) ((|c| + 4 Q) / (8 Q)) on the x 8 scaled
//           coefficient, Q = clip((base scale + 50) / 100, 1, 255), scale = 5000 / quality below 50, else 200 - 2 quality;
//           q Q through the inverse columns (descale 11) and rows (descale 18), + 128, clamped to 0 .. 255 (as
//           libjpeg-turbo's vector code saturates; the portable code's 10-bit wrap was never told apart from it).
//   decode  chroma cropped to ceil(H / 2) x ceil(W / 2), the border sample repeated as context; vertical 3 near + far,
//           then even columns (3 this + left + 8) >> 4, odd (3 this + right + 7) >> 4, first (4 this + 8) >> 4, last
//           (4 this + 7) >> 4; a downsampled width of 1 or 2 is replicated instead (libjpeg's box upsampler).
//           R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
//           B = Y + ((116130 cb + 32768) >> 16), cb, cr centred at 128, clamped.
//   out     SSG_JPEG_OUT_U8_HWC the byte v; SSG_JPEG_OUT_F32_NCHW (float)((double)v / 255.0).
//
// Kernels (256 threads, no atomics; image b of a batch gets the bytes it gets alone):
//   jpeg_tile<TM, HALO>  one workgroup per tile of TM x TM MCUs, TM = 2 (32 x 32 pixels; a grey image has no chroma and
//                    its 8 x 8 MCUs tile the same area).  It reads the tile's pixels once, a 2 x 2 quad per thread (four Y
//                    samples and one chroma sample each), into 8 x 8 blocks in LDS; runs the forward rows, then per
//                    column the forward column, the quantiser and the inverse column in registers, then the inverse
//                    rows: a thread per row or column of a block.  A block is 8 rows of pitch 9 dwords and blocks lie 72
//                    dwords apart: the 32 lanes of a half-wave (4 blocks x 8 rows or columns) then hit 32 different
//                    banks in both directions (bank = 8 (b + r) + r mod 32 for rows, 8 b + c for columns).
//                    HALO = true: the chroma blocks around the tile (4 x 4 instead of 2 x 2) are coded as well, so that
//                    the upsampling's one-sample context is at hand, and the tile's pixels are written: one launch.
//                    HALO = false: the tile's reconstructed Y, Cb and Cr bytes go to the caller's workspace and
//   jpeg_finish      upsamples and converts from there, a pixel per thread: two launches.
//   Measured (profiles/jpeg_codec_tile_ab.txt): the two launches are faster than the one at every shape tried but one
//   (256 x 3 x 64 x 64: 3 % behind), images of a single tile included, and tiles of 2 x 2 MCUs beat 4 x 4 wherever the GPU is not full and match
//   them where it is (a workgroup's time is mostly the latency of its load iterations: one per thread for 2 x 2
//   without the halo, four with it, nine for 4 x 4 with it).  So a colour call takes the two launches and a grey one,
//   which has no chroma to hand over, one; HALO = true and TM = 4 are reachable in the profiling build only.
//   The quantiser divides with a reciprocal: k = (int)((float)n r), r = 1.0f / (float)d, n = |c| + 4 Q < 2^16 and
//   d = 8 Q <= 2040 both exact in fp32; r and the product are each within 2^-23 relative, so |k - n / d| < 1 + 2^-7 and
//   k is floor(n / d) or one beside it; the remainder n - k d then moves k by at most one step to the exact quotient.
#include "ssg_pixel.hpp"

namespace ssg {
namespace jpegcodec {

using pixel::NT;

constexpr int TM_PRODUCT = 2;                  // MCUs per tile side (the profiling build can take 4: SSG_JPEG_TM)
constexpr int ROWP = 9, BLKP = 72;             // dwords per block row, per block
constexpr int CHUNK = 256;                     // images per launch: their qualities travel as kernel arguments

__constant__ unsigned char BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct Args {
  const void *src;
  void *out;
  unsigned char *planes;          // the workspace: per image Y (H W), Cb, Cr (Hc Wc each), `stride` bytes apart
  size_t stride;
  int in_kind, out_kind, C, H, W, Hc, Wc;
  int b0;                         // first image of this launch
  int tiles_x, tiles_y;
  unsigned char quality[CHUNK];
};

__host__ __device__ inline float unit_value(int v) { return (float)((double)v / 255.0); }

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pixel's bytes (a grey image fills r only)
__device__ __forceinline__ void load_pixel(const Args &a, int img, int y, int x, int &r, int &g, int &b) {
  if (a.in_kind == SSG_JPEG_IN_U8_HWC) {
    const unsigned char *p = (const unsigned char *)a.src + (((size_t)img * a.H + y) * a.W + x) * a.C;
    r = p[0];
    if (a.C == 3) g = p[1], b = p[2];
  } else {
    const float *p = (const float *)a.src + ((size_t)img * a.C * a.H + y) * a.W + x;
    const size_t hw = (size_t)a.H * a.W;
    r = (int)rintf(fminf(fmaxf(p[0], 0.f), 1.f) * 255.0f);
    if (a.C == 3) {
      g = (int)rintf(fminf(fmaxf(p[hw], 0.f), 1.f) * 255.0f);
      b = (int)rintf(fminf(fmaxf(p[2 * hw], 0.f), 1.f) * 255.0f);
    }
  }
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
// (each sample is shifted on its own; the downsample sums the shifted values)
__device__ __forceinline__ int chroma_b(int r, int g, int b) {
  return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int chroma_r(int r, int g, int b) {
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// the forward transform of eight values; FIRST: the row pass (scaled up by 4), else the column pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  constexpr int n = FIRST ? 11 : 15;
  int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d[2] = descale(z1 + t13 * 6270, n);
  d[6] = descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
  z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  d[7] = descale(t4 + z1 + z3, n);
  d[5] = descale(t5 + z2 + z4, n);
  d[3] = descale(t6 + z2 + z3, n);
  d[1] = descale(t7 + z1 + z4, n);
}

// the inverse transform of eight values, descaled by N bits
template <int N>
__device__ __forceinline__ void idct8(int (&d)[8]) {
  int z1 = (d[2] + d[6]) * 4433;
  int t2 = z1 - d[6] * 15137, t3 = z1 + d[2] * 6270;
  int t0 = (d[0] + d[4]) * 8192, t1 = (d[0] - d[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
  z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  d[0] = descale(t10 + t3, N), d[7] = descale(t10 - t3, N);
  d[1] = descale(t11 + t2, N), d[6] = descale(t11 - t2, N);
  d[2] = descale(t12 + t1, N), d[5] = descale(t12 - t1, N);
  d[3] = descale(t13 + t0, N), d[4] = descale(t13 - t0, N);
}

// sign(c) ((|c| + 4 Q) / (8 Q)) Q: the coefficient quantised and dequantised; rcp = 1.0f / (float)(8 Q)
__device__ __forceinline__ int requantise(int c, int Q, float rcp) {
  const int n = abs(c) + 4 * Q, d = 8 * Q;
  int k = (int)((float)n * rcp);
  const int rem = n - k * d;
  k += (rem >= d) - (rem < 0);
  return (c < 0 ? -k : k) * Q;
}

// the upsampled chroma value at pixel (y, x); c(cy, cx) is the cropped plane
template <class F>
__device__ __forceinline__ int fancy(F c, int y, int x, int Hc, int Wc) {
  const int cy = y >> 1, cx = x >> 1;
  if (Wc <= 2) return c(cy, cx);
  const int cn = (y & 1) ? min(cy + 1, Hc - 1) : max(cy - 1, 0);
  const int t = 3 * c(cy, cx) + c(cn, cx);
  if (x & 1) {
    if (cx == Wc - 1) return (4 * t + 7) >> 4;
    return (3 * t + 3 * c(cy, cx + 1) + c(cn, cx + 1) + 7) >> 4;
  }
  if (cx == 0) return (4 * t + 8) >> 4;
  return (3 * t + 3 * c(cy, cx - 1) + c(cn, cx - 1) + 8) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ void emit(const Args &a, const float *unit, int img, int y, int x, int ch, int v) {
  if (a.out_kind == SSG_JPEG_OUT_U8_HWC)
    ((unsigned char *)a.out)[(((size_t)img * a.H + y) * a.W + x) * a.C + ch] = (unsigned char)v;
  else
    ((float *)a.out)[(((size_t)img * a.C + ch) * a.H + y) * a.W + x] = unit[v];
}

__device__ __forceinline__ void emit_rgb(const Args &a, const float *unit, int img, int y, int x, int Y, int cb,
                                         int cr) {
  cb -= 128, cr -= 128;
  emit(a, unit, img, y, x, 0, clamp255(Y + ((91881 * cr + 32768) >> 16)));
  emit(a, unit, img, y, x, 1, clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)));
  emit(a, unit, img, y, x, 2, clamp255(Y + ((116130 * cb + 32768) >> 16)));
}

template <int TM, bool HALO>
__global__ __launch_bounds__(NT) void jpeg_tile(Args a) {
  constexpr int TP = 16 * TM;                  // pixels per tile side
  constexpr int NYB = 4 * TM * TM;             // Y blocks of a tile
  constexpr int HB = HALO ? 1 : 0;             // chroma blocks of halo on each side
  constexpr int CB = TM + 2 * HB;              // chroma blocks per side of the coded region
  constexpr int NBLK = NYB + 2 * CB * CB;
  __shared__ int blk[NBLK * BLKP];
  __shared__ int qt[2][64];
  __shared__ float qr[2][64];
  __shared__ float unit[256];
  const int tid = threadIdx.x;
  const int tiles = a.tiles_x * a.tiles_y;
  const int li = blockIdx.x / tiles;           // image within this launch
  const int tile = blockIdx.x - li * tiles;
  const int img = a.b0 + li;
  const int ty0 = (tile / a.tiles_x) * TP, tx0 = (tile % a.tiles_x) * TP;
  const int H = a.H, W = a.W, Hc = a.Hc, Wc = a.Wc;
  const bool colour = a.C == 3;
  const int ncby = (Hc + 7) >> 3, ncbx = (Wc + 7) >> 3;     // chroma blocks of the image
  const int cby0 = (ty0 >> 4) - HB, cbx0 = (tx0 >> 4) - HB; // first chroma block of the coded region (may be -1)

  if (tid < 128) {
    const int quality = a.quality[li];
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int Q = min(max((BASE[tid >> 6][tid & 63] * scale + 50) / 100, 1), 255);
    qt[tid >> 6][tid & 63] = Q;
    qr[tid >> 6][tid & 63] = 1.0f / (float)(8 * Q);
  }
  unit[tid] = unit_value(tid);

  // ---- the tile's samples into blocks ----
  if (colour) {
    for (int item = tid; item < CB * CB * 64; item += NT) {
      const int lr = item / (CB * 8), lc = item - lr * (CB * 8);          // chroma sample within the coded region
      const int cy = cby0 * 8 + lr, cx = cbx0 * 8 + lc;
      const int by = cby0 + (lr >> 3), bx = cbx0 + (lc >> 3);
      if (by < 0 || bx < 0 || by >= ncby || bx >= ncbx) continue;
      const int rr = min(cy, Hc - 1);
      const int y0 = min(2 * rr, H - 1), y1 = min(2 * rr + 1, H - 1), x0 = min(2 * cx, W - 1), x1 = min(2 * cx + 1, W - 1);
      int r[4], g[4], b[4];
      load_pixel(a, img, y0, x0, r[0], g[0], b[0]);
      load_pixel(a, img, y0, x1, r[1], g[1], b[1]);
      load_pixel(a, img, y1, x0, r[2], g[2], b[2]);
      load_pixel(a, img, y1, x1, r[3], g[3], b[3]);
      int sb = 0, sr = 0;
      for (int i = 0; i < 4; ++i) sb += chroma_b(r[i], g[i], b[i]), sr += chroma_r(r[i], g[i], b[i]);
      const int bias = 1 + (cx & 1);
      const int at = ((lr >> 3) * CB + (lc >> 3)) * BLKP + (lr & 7) * ROWP + (lc & 7);
      blk[NYB * BLKP + at] = (sb + bias) >> 2;
      blk[(NYB + CB * CB) * BLKP + at] = (sr + bias) >> 2;
      // the quad's four Y samples, where it lies in the tile proper
      const int qy = lr - 8 * HB, qx = lc - 8 * HB;
      if (qy < 0 || qx < 0 || qy >= 8 * TM || qx >= 8 * TM) continue;
      if (cy >= Hc) {             // below the image the Y rows repeat row H - 1, the chroma rows the last downsampled row
        load_pixel(a, img, H - 1, x0, r[0], g[0], b[0]);
        load_pixel(a, img, H - 1, x1, r[1], g[1], b[1]);
        r[2] = r[0], g[2] = g[0], b[2] = b[0], r[3] = r[1], g[3] = g[1], b[3] = b[1];
      }
      for (int i = 0; i < 4; ++i) {
        const int ly = 2 * qy + (i >> 1), lx = 2 * qx + (i & 1);
        blk[((ly >> 3) * (2 * TM) + (lx >> 3)) * BLKP + (ly & 7) * ROWP + (lx & 7)] = luma(r[i], g[i], b[i]);
      }
    }
  } else {
    for (int item = tid; item < TP * TP; item += NT) {
      const int ly = item / TP, lx = item - ly * TP;
      if (ty0 + (ly & ~7) >= H || tx0 + (lx & ~7) >= W) continue;        // a block wholly outside the image
      int r, g, b;
      load_pixel(a, img, min(ty0 + ly, H - 1), min(tx0 + lx, W - 1), r, g, b);
      blk[((ly >> 3) * (2 * TM) + (lx >> 3)) * BLKP + (ly & 7) * ROWP + (lx & 7)] = r;
    }
  }
  __syncthreads();

  // whether block `bi` of the LDS array holds samples (a Y block wholly outside the image never reaches a pixel and a
  // chroma block outside the image's block grid does not exist), and its table
  auto block_used = [&](int bi, int &comp) {
    if (bi < NYB) {
      comp = 0;
      return ty0 + (bi / (2 * TM)) * 8 < H && tx0 + (bi % (2 * TM)) * 8 < W;
    }
    comp = 1;
    if (!colour) return false;
    const int k = (bi - NYB) % (CB * CB);
    const int by = cby0 + k / CB, bx = cbx0 + k % CB;
    return by >= 0 && bx >= 0 && by < ncby && bx < ncbx;
  };

  // ---- forward rows ----
  for (int item = tid; item < NBLK * 8; item += NT) {
    int comp;
    if (!block_used(item >> 3, comp)) continue;
    int *p = blk + (item >> 3) * BLKP + (item & 7) * ROWP;
    int d[8];
    for (int i = 0; i < 8; ++i) d[i] = p[i] - 128;
    fdct8<true>(d);
    for (int i = 0; i < 8; ++i) p[i] = d[i];
  }
  __syncthreads();
  // ---- forward columns, quantiser, inverse columns ----
  for (int item = tid; item < NBLK * 8; item += NT) {
    int comp;
    if (!block_used(item >> 3, comp)) continue;
    const int c = item & 7;
    int *p = blk + (item >> 3) * BLKP + c;
    int d[8];
    for (int i = 0; i < 8; ++i) d[i] = p[i * ROWP];
    fdct8<false>(d);
    for (int i = 0; i < 8; ++i) d[i] = requantise(d[i], qt[comp][i * 8 + c], qr[comp][i * 8 + c]);
    idct8<11>(d);
    for (int i = 0; i < 8; ++i) p[i * ROWP] = d[i];
  }
  __syncthreads();
  // ---- inverse rows, range limit ----
  for (int item = tid; item < NBLK * 8; item += NT) {
    int comp;
    if (!block_used(item >> 3, comp)) continue;
    int *p = blk + (item >> 3) * BLKP + (item & 7) * ROWP;
    int d[8];
    for (int i = 0; i < 8; ++i) d[i] = p[i];
    idct8<18>(d);
    for (int i = 0; i < 8; ++i) p[i] = clamp255(d[i] + 128);
  }
  __syncthreads();

  auto y_at = [&](int ly, int lx) { return blk[((ly >> 3) * (2 * TM) + (lx >> 3)) * BLKP + (ly & 7) * ROWP + (lx & 7)]; };
  const int th = min(TP, H - ty0), tw = min(TP, W - tx0);
  if (!colour) {
    for (int item = tid; item < th * tw; item += NT) {
      const int ly = item / tw, lx = item - ly * tw;
      emit(a, unit, img, ty0 + ly, tx0 + lx, 0, y_at(ly, lx));
    }
    return;
  }
  if (HALO) {
    for (int item = tid; item < th * tw; item += NT) {
      const int ly = item / tw, lx = item - ly * tw;
      int up[2];
      for (int k = 0; k < 2; ++k) {
        const int *plane = blk + (NYB + k * CB * CB) * BLKP;
        // (cy, cx) of the image's cropped chroma plane, always within one sample of the tile: inside the coded region
        auto c_at = [&](int cy, int cx) {
          const int lr = cy - cby0 * 8, lc = cx - cbx0 * 8;
          return plane[((lr >> 3) * CB + (lc >> 3)) * BLKP + (lr & 7) * ROWP + (lc & 7)];
        };
        up[k] = fancy(c_at, ty0 + ly, tx0 + lx, Hc, Wc);
      }
      emit_rgb(a, unit, img, ty0 + ly, tx0 + lx, y_at(ly, lx), up[0], up[1]);
    }
  } else {
    unsigned char *py = a.planes + (size_t)img * a.stride;
    for (int item = tid; item < th * tw; item += NT) {
      const int ly = item / tw, lx = item - ly * tw;
      py[(size_t)(ty0 + ly) * W + tx0 + lx] = (unsigned char)y_at(ly, lx);
    }
    const int ch = min(TP / 2, Hc - ty0 / 2), cw = min(TP / 2, Wc - tx0 / 2);
    for (int item = tid; item < 2 * ch * cw; item += NT) {
      const int k = item / (ch * cw), rest = item - k * (ch * cw);
      const int lr = rest / cw, lc = rest - lr * cw;
      const int v = blk[(NYB + k * CB * CB + (lr >> 3) * CB + (lc >> 3)) * BLKP + (lr & 7) * ROWP + (lc & 7)];
      py[(size_t)H * W + (size_t)k * Hc * Wc + (size_t)(ty0 / 2 + lr) * Wc + tx0 / 2 + lc] = (unsigned char)v;
    }
  }
}

// the second launch of the two-launch path: a pixel per thread from the reconstructed planes
__global__ __launch_bounds__(NT) void jpeg_finish(Args a, unsigned pixels) {
  __shared__ float unit[256];
  unit[threadIdx.x] = unit_value(threadIdx.x);
  __syncthreads();
  const unsigned at = blockIdx.x * (unsigned)NT + threadIdx.x;          // < 2^31: the entry point bounds B H W C
  if (at >= pixels) return;
  const unsigned hw = (unsigned)a.H * a.W;
  const int li = at / hw, y = (at - li * hw) / a.W, x = at - li * hw - y * a.W;
  const int img = a.b0 + li;
  const unsigned char *py = a.planes + (size_t)img * a.stride;
  int up[2];
  for (int k = 0; k < 2; ++k) {
    const unsigned char *plane = py + (size_t)a.H * a.W + (size_t)k * a.Hc * a.Wc;
    auto c_at = [&](int cy, int cx) { return (int)plane[(size_t)cy * a.Wc + cx]; };
    up[k] = fancy(c_at, y, x, a.Hc, a.Wc);
  }
  emit_rgb(a, unit, img, y, x, py[(size_t)y * a.W + x], up[0], up[1]);
}

// ---------------------------------------------------------------------------------------------------------- host ---
// the profiling build's two A/B switches (profiles/jpeg_codec_tile_ab.txt); the product build takes the defaults
inline int tile_mcus() { return env_int("SSG_JPEG_TM", TM_PRODUCT) == 4 ? 4 : 2; }
inline bool halo_call(int channels) { return channels == 3 && env_int("SSG_JPEG_FUSED", 0) != 0; }

// whether a call hands its planes over in the workspace: every colour call (but under the switch above)
inline bool two_launches(int channels) { return channels == 3 && !halo_call(channels); }

inline size_t image_stride(int H, int W) {
  const size_t hc = (size_t)(H + 1) / 2, wc = (size_t)(W + 1) / 2;
  return align_up((size_t)H * W + 2 * hc * wc, 256);
}

}  // namespace jpegcodec

static size_t jpeg_roundtrip_workspace_bytes(int B, int H, int W, int channels) {
  using namespace jpegcodec;
  if (B < 1 || H < 1 || W < 1 || (channels != 1 && channels != 3)) return 0;
  return two_launches(channels) ? (size_t)B * image_stride(H, W) : 0;
}

static int jpeg_unit_table(float *table) {
  if (!table) return SSG_E_BADARG;
  for (int v = 0; v < 256; ++v) table[v] = jpegcodec::unit_value(v);
  return 0;
}

static int launch_jpeg_roundtrip(const void *in, void *out, int B, int H, int W, int channels, const int *qualities,
                                 int in_layout, int out_epilogue, void *workspace, size_t workspace_bytes, hipStream_t st) {
  using namespace jpegcodec;
  if (!in || !out || in == out || !qualities) return SSG_E_BADARG;
  if (B < 1 || H < 1 || W < 1 || (channels != 1 && channels != 3)) return SSG_E_BADARG;
  if (in_layout != SSG_JPEG_IN_U8_HWC && in_layout != SSG_JPEG_IN_F32_NCHW) return SSG_E_BADARG;
  if (out_epilogue != SSG_JPEG_OUT_U8_HWC && out_epilogue != SSG_JPEG_OUT_F32_NCHW) return SSG_E_BADARG;
  for (int b = 0; b < B; ++b)
    if (qualities[b] < 1 || qualities[b] > 100) return SSG_E_BADARG;
  if ((double)B * H * W * channels >= 2147483648.0) return SSG_E_TOOLARGE;
  const bool planes = two_launches(channels);
  if (planes) {
    if (!workspace) return SSG_E_BADARG;
    if (const int rc = pixel::check_workspace(workspace, workspace_bytes, (size_t)B * image_stride(H, W))) return rc;
  }
  Args a{};
  a.src = in, a.out = out, a.planes = (unsigned char *)workspace, a.stride = image_stride(H, W);
  a.in_kind = in_layout, a.out_kind = out_epilogue, a.C = channels, a.H = H, a.W = W;
  a.Hc = (H + 1) / 2, a.Wc = (W + 1) / 2;
  const int tm = tile_mcus(), TP = 16 * tm;
  a.tiles_x = (W + TP - 1) / TP, a.tiles_y = (H + TP - 1) / TP;
  void (*const tile_kernel)(Args) = halo_call(channels) ? (tm == 2 ? jpeg_tile<2, true> : jpeg_tile<4, true>)
                                                        : (tm == 2 ? jpeg_tile<2, false> : jpeg_tile<4, false>);
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = std::min(CHUNK, B - b0);
    a.b0 = b0;
    for (int i = 0; i < nb; ++i) a.quality[i] = (unsigned char)qualities[b0 + i];
    // tiles x images <= pixels < 2^31
    const unsigned grid = (unsigned)((size_t)a.tiles_x * a.tiles_y * nb);
    hipLaunchKernelGGL(tile_kernel, dim3(grid), dim3(NT), 0, st, a);
    if (planes) {
      if (const hipError_t e = hipGetLastError()) return (int)e;
      const unsigned pixels = (unsigned)((size_t)nb * H * W);
      hipLaunchKernelGGL(jpegcodec::jpeg_finish, dim3((pixels + NT - 1) / NT), dim3(NT), 0, st, a, pixels);
    }
    if (const hipError_t e = hipGetLastError()) return (int)e;
  }
  return 0;
}

}  // namespace ssg

extern "C" {

size_t ssg_jpeg_roundtrip_workspace_bytes(int B, int H, int W, int channels) {
  return ssg::jpeg_roundtrip_workspace_bytes(B, H, W, channels);
}

int ssg_jpeg_unit_table(float *table) { return ssg::jpeg_unit_table(table); }

int ssg_jpeg_roundtrip(const void *in, void *out, int B, int H, int W, int channels, const int *qualities,
                       int in_layout, int out_epilogue, void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  return ssg::launch_jpeg_roundtrip(in, out, B, H, W, channels, qualities, in_layout, out_epilogue, workspace,
                                    workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
