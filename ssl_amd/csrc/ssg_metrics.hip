// The validation metrics on the GPU: basicsr/metrics/psnr_ssim.py (calculate_psnr :12-48, calculate_ssim :85-128, _ssim
// :170-198) on what basicsr/utils/img_util.py:37-93 (tensor2img) hands them, with metric_util.py:32-45 (to_y_channel)
// and color_util.py:38-67,129-183 (bgr2ycbcr, y_only) in between.  Two images of one shape in, PSNR and SSIM per image
// out; nothing is copied to the host and nothing of image size is written.
//
// Contract (every step restated operation by operation: this file is compiled with -ffp-contract=off):
//   quantise  float input only: q = rint(fl32(clamp(x, 0, 1) * 255.0f)), ties to even; uint8 input is q already.  A
//             float image is RGB and is read as BGR (plane p reads channel C - 1 - p); uint8 images are BGR.  NaN is
//             unspecified (the reference's uint8 cast of NaN is undefined).
//   crop      `crop` pixels from each side: Hc = H - 2 crop, Wc = W - 2 crop
//   planes    y_channel, C = 3:  v_c = fl32(q_c / 255.0f);  t = ((24.966 v_b + 128.553 v_g) + 65.481 v_r) + 16.0 in
//                                fp64, no fma;  plane = fl32(fl32(t / 255.0) * 255.0f): one plane
//             y_channel, C = 1:  plane = fl32(fl32(q / 255.0f) * 255.0f)
//             otherwise:         the C planes are the integers q
//   PSNR      mse = (sum over planes and pixels of fl64(d * d), d = plane_a - plane_b in fp64) / (P Hc Wc);
//             10 log10(255^2 / mse), +inf where mse == 0.  Without y_channel the sum is counted in 64-bit integers.
//   SSIM      per plane the five moments E[x], E[y], E[x^2], E[y^2], E[xy] under the 11 x 11 window g_i g_j,
//             g_i = exp(-(i - 5)^2 / 4.5) / sum, on the 'valid' region Hm x Wm = (Hc - 10) x (Wc - 10); c1 = 6.5025,
//             c2 = 58.5225; map = ((2 mu1 mu2 + c1)(2 s12 + c2)) / ((mu1^2 + mu2^2 + c1)(s1 + s2 + c2)) with
//             s1 = E[x^2] - mu1^2, s2 = E[y^2] - mu2^2, s12 = E[xy] - mu1 mu2; the mean over the map and the planes.
//             All of it fp64.
//
// Two launches, no atomics, no ticket, every sum in a fixed order (bit-reproducible):
//   metric_tiles  a 32 x 16 tile of the map per workgroup pass, grid (min(tiles per image, 512), B); a workgroup walks
//                 the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its image (planes, then tile rows, then tile
//                 columns).  Per tile: both images' 42 x 26 haloed planes are formed at load time (quantise, crop, Y)
//                 into LDS as fp32 -- every plane value is exact in fp32 -- each input byte read once per tile; the
//                 squared differences of the pixels the tile OWNS (its 32 x 16 centre, widened to the image's border in
//                 the first and last tile row / column, so every pixel has one owner) are summed at load; the row pass
//                 forms the five 11-tap moments in fp64 registers, LDS -> LDS; the column pass and the map value LDS ->
//                 registers.  One {map sum, squared-difference sum, integer squared-difference sum} per workgroup goes
//                 to the workspace.
//   metric_fold   one workgroup per image folds that image's partials in index order and writes the four results.
//   LDS: xa, xb fp32 [26][43]; mid fp64 [5][26][33].  Lanes run along the tile's 32 columns in every pass, so a 32-lane
//   group of ds_read_b32 reads 32 consecutive dwords (32 banks) and of ds_read_b64 32 consecutive fp64 = 64 consecutive
//   dwords (all 64 banks once), whatever the row stride: conflict-free.  The strides are odd (43 dwords, 33 fp64 = 66
//   dwords) so that the two 32-lane groups of a wave, which hold consecutive rows, start 66 mod 64 = 2 banks apart
//   instead of on the same bank, and the five moment planes (26 * 33 fp64 apart) do not line up either.
#include <math.h>

#include "ssg_pixel.hpp"

namespace ssg {
namespace metric {

using pixel::NT;
using pixel::check_workspace;
using pixel::plane_value;

constexpr int TW = 32, TH = 16;          // map tile
constexpr int R = 5, K = 2 * R + 1;      // the 11-tap window
constexpr int IW = TW + 2 * R, IH = TH + 2 * R;   // 42 x 26 haloed tile
constexpr int IWS = IW + 1;              // 43: fp32 row stride
constexpr int MWS = TW + 1;              // 33: fp64 row stride of the row pass's output
constexpr int MAX_WG = 512;              // workgroups per image

struct Args {
  const void *a, *b;    // the two images
  float *planes;        // metric_planes: (B,P,Hc,Wc)
  double *p_map;        // (B, wg) partial sums of the map
  double *p_sq;         // (B, wg) partial sums of the squared plane differences (y_channel)
  unsigned long long *p_int;   // (B, wg) the same in integers (no y_channel)
  double *out;          // (B,4)
  double g[K];
  int kind, B, C, H, W, crop, ych;
  int P, Hc, Wc, Hm, Wm;
  int ntx, nty, tiles;  // tiles per row, per column, per image (P nty ntx)
  int wg;               // workgroups per image
};

__global__ __launch_bounds__(NT) void metric_planes(Args a) {
  const size_t n = (size_t)a.B * a.P * a.Hc * a.Wc;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const int x = (int)(i % a.Wc);
    size_t r = i / a.Wc;
    const int y = (int)(r % a.Hc);
    r /= a.Hc;
    const int p = (int)(r % a.P), img = (int)(r / a.P);
    a.planes[i] = plane_value(a.a, a, img, p, y + a.crop, x + a.crop);
  }
}

// fixed-order workgroup sum (pixel::block_sum's order) of one value; `sh` is this sum's own NT / 64 slots
template <class T>
__device__ __forceinline__ T wg_sum(T v, T *sh) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = sh[0];
  for (int i = 1; i < NT / 64; ++i) s += sh[i];
  return s;
}

__global__ __launch_bounds__(NT) void metric_tiles(Args a) {
  __shared__ float xa[IH * IWS], xb[IH * IWS];
  __shared__ double mid[5 * IH * MWS];
  __shared__ double sh_map[NT / 64], sh_sq[NT / 64];
  __shared__ unsigned long long sh_int[NT / 64];
  const int img = blockIdx.y;
  const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
  double s_map = 0.0, s_sq = 0.0;
  unsigned long long s_int = 0;
  for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    const int per = a.ntx * a.nty;
    const int p = t / per, r = t - p * per, ty = r / a.ntx, tx = r - ty * a.ntx;
    const int oy0 = ty * TH, ox0 = tx * TW;
    // ---- load: quantise, crop, Y; squared differences of the pixels this tile owns ----
    for (int e = threadIdx.x; e < IH * IW; e += NT) {
      const int ly = e / IW, lx = e - ly * IW;
      const int y = oy0 + ly, x = ox0 + lx;    // in the cropped image
      float va = 0.f, vb = 0.f;
      if (y < a.Hc && x < a.Wc) {
        va = plane_value(a.a, a, img, p, y + a.crop, x + a.crop);
        vb = plane_value(a.b, a, img, p, y + a.crop, x + a.crop);
        const bool own = (ly >= R || ty == 0) && (ly < R + TH || ty == a.nty - 1) && (lx >= R || tx == 0) &&
                         (lx < R + TW || tx == a.ntx - 1);
        if (own) {
          if (a.ych) {
            const double d = (double)va - (double)vb;
            s_sq += d * d;
          } else {
            const int d = (int)va - (int)vb;
            s_int += (unsigned long long)(d * d);
          }
        }
      }
      xa[ly * IWS + lx] = va;
      xb[ly * IWS + lx] = vb;
    }
    __syncthreads();
    // ---- row pass: the five moments along x, fp64, taps in index order ----
    for (int e = threadIdx.x; e < IH * TW; e += NT) {
      const int iy = e / TW, ox = e - iy * TW;
      const float *ra = xa + iy * IWS + ox, *rb = xb + iy * IWS + ox;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double u = (double)ra[j], v = (double)rb[j], w = a.g[j];
        m0 += w * u;
        m1 += w * v;
        m2 += w * (u * u);
        m3 += w * (v * v);
        m4 += w * (u * v);
      }
      double *o = mid + iy * MWS + ox;
      o[0 * IH * MWS] = m0;
      o[1 * IH * MWS] = m1;
      o[2 * IH * MWS] = m2;
      o[3 * IH * MWS] = m3;
      o[4 * IH * MWS] = m4;
    }
    __syncthreads();
    // ---- column pass and the map ----
    for (int e = threadIdx.x; e < TH * TW; e += NT) {
      const int oy = e / TW, ox = e - oy * TW;
      if (oy0 + oy < a.Hm && ox0 + ox < a.Wm) {
        const double *c = mid + oy * MWS + ox;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          const double w = a.g[i];
          m0 += w * c[0 * IH * MWS + i * MWS];
          m1 += w * c[1 * IH * MWS + i * MWS];
          m2 += w * c[2 * IH * MWS + i * MWS];
          m3 += w * c[3 * IH * MWS + i * MWS];
          m4 += w * c[4 * IH * MWS + i * MWS];
        }
        const double mu1_sq = m0 * m0, mu2_sq = m1 * m1, mu12 = m0 * m1;
        const double s1 = m2 - mu1_sq, s2 = m3 - mu2_sq, s12 = m4 - mu12;
        s_map += ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2));
      }
    }
    __syncthreads();   // the next tile overwrites xa, xb and mid
  }
  const double t_map = wg_sum(s_map, sh_map), t_sq = wg_sum(s_sq, sh_sq);
  const unsigned long long t_int = wg_sum(s_int, sh_int);
  if (threadIdx.x == 0) {
    const size_t at = (size_t)img * a.wg + blockIdx.x;
    a.p_map[at] = t_map;
    a.p_sq[at] = t_sq;
    a.p_int[at] = t_int;
  }
}

__global__ __launch_bounds__(NT) void metric_fold(Args a) {
  __shared__ double sh_map[NT / 64], sh_sq[NT / 64];
  __shared__ unsigned long long sh_int[NT / 64];
  const size_t base = (size_t)blockIdx.x * a.wg;
  double s_map = 0.0, s_sq = 0.0;
  unsigned long long s_int = 0;
  for (int i = threadIdx.x; i < a.wg; i += NT) {
    s_map += a.p_map[base + i];
    s_sq += a.p_sq[base + i];
    s_int += a.p_int[base + i];
  }
  const double t_map = wg_sum(s_map, sh_map), t_sq = wg_sum(s_sq, sh_sq);
  const unsigned long long t_int = wg_sum(s_int, sh_int);
  if (threadIdx.x == 0) {
    const double n = (double)a.P * a.Hc * a.Wc;
    const double sq = a.ych ? t_sq : (double)t_int;
    const double mse = sq / n;
    double *o = a.out + (size_t)blockIdx.x * 4;
    o[0] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(255.0 * 255.0 / mse);
    o[1] = t_map / ((double)a.P * a.Hm * a.Wm);
    o[2] = sq;
    o[3] = n;
  }
}

// ---------------------------------------------------------------------------------------------------------- host ---
// argument checks shared by the entry points, in the order the header documents; min_side is the shortest cropped side
inline int check_shape(int kind, int B, int C, int H, int W, int crop, int min_side) {
  if (B <= 0 || H <= 0 || W <= 0 || crop < 0) return SSG_E_BADARG;
  if (C != 1 && C != 3) return SSG_E_BADARG;
  if (kind != SSG_METRIC_F32_RGB && kind != SSG_METRIC_U8_HWC && kind != SSG_METRIC_U8_CHW) return SSG_E_BADARG;
  if (B > 65535 || (double)B * C * H * W >= 2147483648.0) return SSG_E_TOOLARGE;
  if ((long)H - 2L * crop < min_side || (long)W - 2L * crop < min_side) return SSG_E_IMAGESMALL;
  return 0;
}

inline void geometry(Args &a, int kind, int B, int C, int H, int W, int crop, int ych) {
  a.kind = kind, a.B = B, a.C = C, a.H = H, a.W = W, a.crop = crop, a.ych = ych != 0;
  a.P = a.ych ? 1 : C;
  a.Hc = H - 2 * crop, a.Wc = W - 2 * crop;
  a.Hm = a.Hc - 2 * R, a.Wm = a.Wc - 2 * R;
  a.ntx = (a.Wm + TW - 1) / TW, a.nty = (a.Hm + TH - 1) / TH;
  a.tiles = a.P * a.ntx * a.nty;        // < 2^31: every tile holds a pixel
  a.wg = a.tiles < MAX_WG ? a.tiles : MAX_WG;
  double sum = 0.0;
  for (int i = 0; i < K; ++i) sum += a.g[i] = exp(-(double)((i - R) * (i - R)) / (2.0 * 1.5 * 1.5));
  for (int i = 0; i < K; ++i) a.g[i] /= sum;
}

struct Layout {
  size_t map, sq, cnt, total;
};

inline Layout layout(const Args &a) {
  Layout L;
  Carver c;
  const size_t n = (size_t)a.B * a.wg;
  L.map = c.take(sizeof(double) * n);
  L.sq = c.take(sizeof(double) * n);
  L.cnt = c.take(sizeof(unsigned long long) * n);
  L.total = c.end;
  return L;
}

}  // namespace metric

static size_t metric_workspace_bytes(int B, int C, int H, int W, int crop) {
  using namespace metric;
  if (check_shape(SSG_METRIC_F32_RGB, B, C, H, W, crop, K)) return 0;
  Args a{};
  geometry(a, SSG_METRIC_F32_RGB, B, C, H, W, crop, 0);   // (the plain planes: the most tiles a shape has)
  return layout(a).total;
}

}  // namespace ssg

using namespace ssg::metric;

extern "C" {

size_t ssg_metric_workspace_bytes(int B, int C, int H, int W, int crop_border) {
  return ssg::metric_workspace_bytes(B, C, H, W, crop_border);
}

int ssg_psnr_ssim(const void *a_img, const void *b_img, int kind, int B, int C, int H, int W, int crop_border,
                  int y_channel, double *out, void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  if (!a_img || !b_img || !out || !workspace) return SSG_E_BADARG;
  const int rc = check_shape(kind, B, C, H, W, crop_border, K);
  if (rc) return rc;
  Args a{};
  geometry(a, kind, B, C, H, W, crop_border, y_channel);
  const Layout L = layout(a);
  const int ws_rc = check_workspace(workspace, workspace_bytes, L.total);
  if (ws_rc) return ws_rc;
  a.a = a_img;
  a.b = b_img;
  a.out = out;
  a.p_map = (double *)((char *)workspace + L.map);
  a.p_sq = (double *)((char *)workspace + L.sq);
  a.p_int = (unsigned long long *)((char *)workspace + L.cnt);
  hipLaunchKernelGGL(metric_tiles, dim3((unsigned)a.wg, (unsigned)B), dim3(NT), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(metric_fold, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int ssg_metric_planes(const void *img, int kind, int B, int C, int H, int W, int crop_border, int y_channel,
                      float *planes_out, ssg_stream_t stream) {
  if (!img || !planes_out) return SSG_E_BADARG;
  const int rc = check_shape(kind, B, C, H, W, crop_border, 1);
  if (rc) return rc;
  Args a{};
  geometry(a, kind, B, C, H, W, crop_border, y_channel);
  a.a = img;
  a.planes = planes_out;
  const size_t n = (size_t)B * a.P * a.Hc * a.Wc;
  const size_t blocks = (n + NT - 1) / NT;
  hipLaunchKernelGGL(metric_planes, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(NT), 0, (hipStream_t)stream,
                     a);
  return (int)hipGetLastError();
}

}  // extern "C"
