// What the pixel-loss kernels share (ssg_ldl.hip, ssg_bbl.hip, ssg_bp.hip): the workgroup size, sgn, the fixed-order fp64
// workgroup sum, the reflect-padded 32 x 16 tile of the two local-variance kernels (ldl_map, flat_mask) and the
// workspace test that ends their entry points' argument checks, and the metric files' (ssg_metrics.hip, ssg_niqe.hip)
// quantised / Y plane value.  One definition each: a fix reaches every file.
#pragma once
#include "../../include/ssg_hip.h"

#include "ssg_host.hpp"

namespace ssg {
namespace pixel {

constexpr int NT = 256;                  // threads per workgroup, every kernel of the three files

__device__ __forceinline__ float sgnf(float x) { return (float)((x > 0.f) - (x < 0.f)); }

// fixed-order workgroup sum of one fp64 value (every thread must call it; thread 0's result is the sum)
__device__ __forceinline__ double block_sum(double v, double *sh) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
  for (int i = 1; i < NT / 64; ++i) s += sh[i];
  return s;
}

// ---- the haloed tile of ldl_map / ldl_grad / flat_mask ----
constexpr int TW = 32, TH = 16;          // output tile: 2 pixels per thread
constexpr int KMAX = 15, RMAX = KMAX / 2;
constexpr int LH = TH + 2 * RMAX;        // 30 tile rows with the largest halo
constexpr int LW = TW + 2 * RMAX + 1;    // 47: row stride of the haloed tiles (+1 breaks the power-of-two stride)

// reflect (pad < n) and clamp: coordinates beyond the padded range only occur in tile rows / columns that lie outside
// the image and are never used; the clamp keeps their loads in bounds
__device__ __forceinline__ int reflect_clamp(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

// fills tile rows / columns [0, TH + 2R) x [0, TW + 2R) with value(offset of the reflected pixel in its H x W plane)
// for the output tile at (ty0, tx0); the caller's barrier follows
template <class F>
__device__ __forceinline__ void load_halo_tile(float (&tile)[LH][LW], int ty0, int tx0, int R, int H, int W, F value) {
  const int lw = TW + 2 * R, lh = TH + 2 * R;
  for (int i = threadIdx.x; i < lh * lw; i += NT) {
    const int ly = i / lw, lx = i - ly * lw;
    tile[ly][lx] = value(reflect_clamp(ty0 - R + ly, H) * W + reflect_clamp(tx0 - R + lx, W));
  }
}

// ---- the metrics' planes (ssg_metrics.hip, ssg_niqe.hip) ----
// plane p of image n at (y, x) of the UNCROPPED image, after quantise and Y; Args holds kind, C, H, W and ych
template <class Args>
__device__ __forceinline__ float plane_value(const void *img, const Args &a, int n, int p, int y, int x) {
  const size_t hw = (size_t)a.H * a.W;
  const size_t at = (size_t)y * a.W + x;
  float q[3];
  const int nq = a.ych ? a.C : 1;       // Y reads every channel, a plain plane its own
  for (int i = 0; i < nq; ++i) {
    const int c = a.ych ? i : p;        // BGR index
    if (a.kind == SSG_METRIC_F32_RGB) {
      const float v = ((const float *)img)[((size_t)n * a.C + (a.C - 1 - c)) * hw + at];
      q[i] = rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);
    } else if (a.kind == SSG_METRIC_U8_HWC) {
      q[i] = (float)((const uint8_t *)img)[((size_t)n * hw + at) * a.C + c];
    } else {
      q[i] = (float)((const uint8_t *)img)[((size_t)n * a.C + c) * hw + at];
    }
  }
  if (!a.ych) return q[0];
  if (a.C == 1) return (q[0] / 255.0f) * 255.0f;
  const double vb = (double)(q[0] / 255.0f), vg = (double)(q[1] / 255.0f), vr = (double)(q[2] / 255.0f);
  const double t = ((24.966 * vb + 128.553 * vg) + 65.481 * vr) + 16.0;
  return (float)(t / 255.0) * 255.0f;
}

// ---- host ----
// the end of the argument checks of every entry point that takes a workspace: too small, then misaligned (the fp64
// partials in it are read as 16-byte pairs)
inline int check_workspace(const void *ws, size_t ws_bytes, size_t needed) {
  if (ws_bytes < needed) return SSG_E_WORKSPACE;
  if (unaligned(ws, 16)) return SSG_E_ALIGN;
  return 0;
}

}  // namespace pixel
}  // namespace ssg
