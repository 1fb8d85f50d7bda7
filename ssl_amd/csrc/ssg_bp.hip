// BebyGAN's back-projection loss on the GPU: GAN-Based-SR/basicsr/models/bebyganssl_model.py:727-731
// (l_pix_bp = L1Loss(imresize(output, 1 / scale), lq)) and the imresize it calls (:375-469) on its integer-factor path
// (discrete_kernel -> downsampling_2d, :133-162, :351-373): MATLAB's antialiased bicubic.
//
// Contract (x (P,H,W) fp32 planes, s the integer factor 2, 3 or 4; K = 4s for even s, 4s - 1 for odd s; p = (K - s) / 2):
//   taps   w_i = c(r_i) / sum_j c(r_j), r_i = (i - (K-1)/2) / s, c the Keys cubic with a = -0.5; formed on the host in
//          fp64 and rounded once to fp32.  The 2-D tap is w_i w_j (the passes below are separable).
//   pad    symmetric, p pixels per side: index -1-i reads pixel i, n+i reads n-1-i (the edge pixel twice)
//   y[oy,ox] = sum_{i,j<K} w_i w_j x~[s oy + i - p, s ox + j - p],  h = H / s, w = W / s (floor);  H, W >= p
//   loss   = loss_weight mean |y - lq| (or the sum);  sgn(0) = 0;  lq carries no gradient
//   grad_x = loss_weight / M  K^T sgn(y - lq): the exact adjoint of pad + strided correlation, formed as a GATHER.  Per
//          axis a pixel i has the padded copies q = p + i, p - 1 - i (i < p) and p + 2n - 1 - i (i >= n - p) -- for
//          p <= n < 2p one pixel has all three -- and copy q lies in the windows o with 0 <= q - s o < K, at most 4.
//          The effective per-axis weight of (i, o) is the sum over the copies, so the two axes stay separable.
//
// Two launches per loss call, no atomics, every sum in a fixed order (bit-reproducible), no padded copy anywhere:
//   bp_fwd<S>  a 16 x 8 output tile per workgroup pass: the (16 S + K - S) x (8 S + K - S) input tile is loaded once into
//              LDS with the mirror applied to the index, the row pass runs LDS -> LDS, the column pass LDS -> registers.
//              Writes y (optional), sgn(y - lq) and one fp64 partial of sum |y - lq| per workgroup; a workgroup walks
//              tiles blockIdx, blockIdx + gridDim, ... (at most 4,096 workgroups, so the partials take 32 KiB).
//              LDS layout: lanes of the row pass run along the tile's ROWS (odd row stride: conflict-free, where lanes
//              along the output columns would read stride S = 4 dwords, a 4-way conflict) and write the intermediate
//              transposed ([ox][iy], odd stride), which the column pass reads with lanes along ox.
//   bp_bwd<S>  a 64 x 32 gradient tile per workgroup: the <= 20 x 12 (s = 4) upstream values its pixels' copies touch
//              are loaded into LDS (the arrays are one longer per side: 21 x 13), the column gather runs LDS -> LDS, the row gather LDS -> global.  Workgroup 0 also
//              folds the forward's partials, in index order, into the loss.
#include <math.h>

#include "ssg_pixel.hpp"

namespace ssg {
namespace bp {

using pixel::NT;               // (by name: this file has a KMAX of its own, the longest tap row)
using pixel::block_sum;
using pixel::check_workspace;
using pixel::sgnf;

constexpr int OTW = 16;        // forward: output tile
constexpr int OTH = 8;
constexpr int GW = 64;         // backward: gradient tile
constexpr int GH = 32;
constexpr int MAX_FWD_WG = 4096;
constexpr int KMAX = 16;

constexpr int taps_of(int s) { return s % 2 ? 4 * s - 1 : 4 * s; }

struct Args {
  const float *x;       // (P,H,W)
  const float *lq;      // (P,h,w), null for the plain downsample
  float *y;             // (P,h,w), nullable
  float *sg;            // (P,h,w) sgn(y - lq), nullable
  double *part;         // one per forward workgroup
  float *loss;          // 1 float, nullable
  const float *gy;      // backward: upstream (P,h,w)
  float *grad;          // backward: (P,H,W)
  float tap[KMAX];
  float scale;          // the gradient's factor (1 for the generic backward)
  double loss_scale;
  int P, H, W, ho, wo;
  int ftx, fty, ftiles, fwg;   // forward tiles per row / column, in all, and the workgroups that walk them
  int btx, bty;                // backward tiles
};

// symmetric padding: -1-i -> i, n+i -> n-1-i.  Coordinates beyond the padded range only occur in tile rows / columns
// that no output of the image uses; the clamp keeps their loads in bounds.
__device__ __forceinline__ int sym_clamp(int i, int n) {
  i = i < 0 ? -1 - i : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return min(max(i, 0), n - 1);
}

// ------------------------------------------------------------------------------------------------------ forward ---
template <int S>
__global__ __launch_bounds__(NT) void bp_fwd(Args a) {
  constexpr int K = taps_of(S), PAD = (K - S) / 2;
  constexpr int IW = OTW * S + K - S, IH = OTH * S + K - S;
  constexpr int IWP = IW | 1, IHP = IH | 1;
  __shared__ float tin[IH * IWP];      // the input tile, [iy][ix]
  __shared__ float mid[OTW * IHP];     // after the row pass, transposed: [ox][iy]
  __shared__ double sh[NT / 64];
  double lsum = 0.0;
  for (int t = blockIdx.x; t < a.ftiles; t += gridDim.x) {
    const int per = a.ftx * a.fty;
    const int pl = t / per, r = t - pl * per, ty = r / a.ftx, tx = r - ty * a.ftx;
    const int oy0 = ty * OTH, ox0 = tx * OTW;
    const float *xp = a.x + (size_t)pl * a.H * a.W;
    for (int e = threadIdx.x; e < IH * IW; e += NT) {
      const int ly = e / IW, lx = e - ly * IW;
      tin[ly * IWP + lx] =
          xp[(size_t)sym_clamp(oy0 * S - PAD + ly, a.H) * a.W + sym_clamp(ox0 * S - PAD + lx, a.W)];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < IH * OTW; e += NT) {
      const int ox = e / IH, iy = e - ox * IH;
      const float *row = tin + iy * IWP + ox * S;
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < K; ++j) v += a.tap[j] * row[j];
      mid[ox * IHP + iy] = v;
    }
    __syncthreads();
    if (threadIdx.x < OTW * OTH) {
      const int oy = threadIdx.x / OTW, ox = threadIdx.x - oy * OTW;
      const int gy = oy0 + oy, gx = ox0 + ox;
      if (gy < a.ho && gx < a.wo) {
        const float *col = mid + ox * IHP + oy * S;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) v += a.tap[i] * col[i];
        const size_t at = ((size_t)pl * a.ho + gy) * a.wo + gx;
        if (a.y) a.y[at] = v;
        if (a.lq) {
          const float d = v - a.lq[at];
          lsum += (double)fabsf(d);
          if (a.sg) a.sg[at] = sgnf(d);
        }
      }
    }
    __syncthreads();   // the next tile overwrites tin and mid
  }
  if (a.part) {
    const double s = block_sum(lsum, sh);
    if (threadIdx.x == 0) a.part[blockIdx.x] = s;
  }
}

// ----------------------------------------------------------------------------------------------------- backward ---
// sum over the windows o (o_lo <= o <= o_last) that hold padded coordinate q: w[q - S o] src[(o - o_lo) stride]
template <int S, int K>
__device__ __forceinline__ float windows_of(const float *wl, const float *src, int stride, int q, int o_lo,
                                            int o_last) {
  float acc = 0.f;
  for (int o = min(q / S, o_last); o >= o_lo && q - S * o < K; --o) acc += wl[q - S * o] * src[(o - o_lo) * stride];
  return acc;
}

// pixel i of a side of n pixels: its direct copy, then the mirror in front, then the mirror behind
template <int S, int K>
__device__ __forceinline__ float copies_of(const float *wl, const float *src, int stride, int i, int n, int o_lo,
                                           int o_last) {
  constexpr int PAD = (K - S) / 2;
  float acc = windows_of<S, K>(wl, src, stride, PAD + i, o_lo, o_last);
  if (i < PAD) acc += windows_of<S, K>(wl, src, stride, PAD - 1 - i, o_lo, o_last);
  if (i >= n - PAD) acc += windows_of<S, K>(wl, src, stride, PAD + 2 * n - 1 - i, o_lo, o_last);
  return acc;
}

// the windows a run of pixels [i0, i1] of a side touches: [lo, hi].  The mirrors add none: a pixel in front of PAD has
// lo = 0 already and its mirror lies in front of its direct copy; a pixel behind n - PAD has hi = n_o - 1 already.
template <int S, int K>
__device__ __forceinline__ void window_range(int i0, int i1, int n_o, int &lo, int &hi) {
  constexpr int PAD = (K - S) / 2;
  const int u = PAD + i0 - K + 1;
  lo = u > 0 ? (u + S - 1) / S : 0;
  hi = min((PAD + i1) / S, n_o - 1);
}

template <int S>
__global__ __launch_bounds__(NT) void bp_bwd(Args a) {
  constexpr int K = taps_of(S);
  constexpr int ONX = (GW + K - 2) / S + 2, ONY = (GH + K - 2) / S + 2, ONXP = ONX | 1;
  __shared__ float gs[ONY * ONXP];    // the upstream values, [oy][ox]
  __shared__ float tm[GH * ONXP];     // after the column gather, [iy][ox]
  __shared__ float wl[KMAX];
  __shared__ double sh[NT / 64];
  if (a.grad) {
    const int per = a.btx * a.bty;
    const int pl = blockIdx.x / per, r = blockIdx.x - pl * per, ty = r / a.btx, tx = r - ty * a.btx;
    const int iy0 = ty * GH, ix0 = tx * GW;
    int oy_lo, oy_hi, ox_lo, ox_hi;
    window_range<S, K>(iy0, min(iy0 + GH, a.H) - 1, a.ho, oy_lo, oy_hi);
    window_range<S, K>(ix0, min(ix0 + GW, a.W) - 1, a.wo, ox_lo, ox_hi);
    const int noy = oy_hi - oy_lo + 1, nox = ox_hi - ox_lo + 1;   // <= ONY - 1, ONX - 1
    if (threadIdx.x < KMAX) wl[threadIdx.x] = a.tap[threadIdx.x];
    const float *gp = a.gy + (size_t)pl * a.ho * a.wo;
    for (int e = threadIdx.x; e < noy * nox; e += NT) {
      const int ly = e / nox, lx = e - ly * nox;
      gs[ly * ONXP + lx] = gp[(size_t)(oy_lo + ly) * a.wo + ox_lo + lx];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < GH * nox; e += NT) {
      const int ly = e / nox, lx = e - ly * nox;
      if (iy0 + ly < a.H) tm[ly * ONXP + lx] = copies_of<S, K>(wl, gs + lx, ONXP, iy0 + ly, a.H, oy_lo, a.ho - 1);
    }
    __syncthreads();
    float *out = a.grad + (size_t)pl * a.H * a.W;
    for (int e = threadIdx.x; e < GH * GW; e += NT) {
      const int ly = e / GW, lx = e - ly * GW;
      const int iy = iy0 + ly, ix = ix0 + lx;
      if (iy < a.H && ix < a.W)
        out[(size_t)iy * a.W + ix] = a.scale * copies_of<S, K>(wl, tm + ly * ONXP, 1, ix, a.W, ox_lo, a.wo - 1);
    }
  }
  if (a.loss && blockIdx.x == 0) {   // (workgroup-uniform)
    double l = 0.0;
    for (int i = threadIdx.x; i < a.fwg; i += NT) l += a.part[i];
    __syncthreads();
    l = block_sum(l, sh);
    if (threadIdx.x == 0) a.loss[0] = (float)(a.loss_scale * l);
  }
}

// ---------------------------------------------------------------------------------------------------------- host ---
inline double keys(double r) {
  const double a = -0.5, x = fabs(r);
  if (x <= 1.0) return (a + 2) * x * x * x - (a + 3) * x * x + 1;
  if (x <= 2.0) return a * x * x * x - 5 * a * x * x + 8 * a * x - 4 * a;
  return 0.0;
}

// argument checks shared by the entry points, in the order the header documents
inline int check_shape(int P, int H, int W, int s) {
  if (P <= 0 || H <= 0 || W <= 0 || s < 2) return SSG_E_BADARG;
  if (s > 4 || (double)P * H * W >= 2147483648.0) return SSG_E_TOOLARGE;
  const int pad = (taps_of(s) - s) / 2;
  if (H < pad || W < pad) return SSG_E_IMAGESMALL;
  return 0;
}

inline void geometry(Args &a, int P, int H, int W, int s) {
  a.P = P, a.H = H, a.W = W, a.ho = H / s, a.wo = W / s;
  a.ftx = (a.wo + OTW - 1) / OTW, a.fty = (a.ho + OTH - 1) / OTH;
  const long tiles = (long)P * a.ftx * a.fty;   // < 2^31: every tile holds an output, an output s^2 pixels
  a.ftiles = (int)tiles;
  a.fwg = tiles < MAX_FWD_WG ? (int)tiles : MAX_FWD_WG;
  a.btx = (W + GW - 1) / GW, a.bty = (H + GH - 1) / GH;
  const int K = taps_of(s);
  double c[KMAX], sum = 0.0;
  for (int i = 0; i < K; ++i) sum += c[i] = keys((i - (K - 1) / 2.0) / s);
  for (int i = 0; i < KMAX; ++i) a.tap[i] = i < K ? (float)(c[i] / sum) : 0.f;
}

struct Layout {
  size_t sg, part, total;
};

inline Layout layout(const Args &a) {
  Layout L;
  Carver c;
  L.sg = c.take(sizeof(float) * (size_t)a.P * a.ho * a.wo);
  L.part = c.take(sizeof(double) * (size_t)a.fwg);
  L.total = c.end;
  return L;
}

inline void launch_fwd(const Args &a, int s, hipStream_t st) {
  const dim3 grid((unsigned)a.fwg);
  if (s == 2)
    hipLaunchKernelGGL((bp_fwd<2>), grid, dim3(NT), 0, st, a);
  else if (s == 3)
    hipLaunchKernelGGL((bp_fwd<3>), grid, dim3(NT), 0, st, a);
  else
    hipLaunchKernelGGL((bp_fwd<4>), grid, dim3(NT), 0, st, a);
}

inline void launch_bwd(const Args &a, int s, hipStream_t st) {
  const dim3 grid(a.grad ? (unsigned)a.P * a.btx * a.bty : 1u);
  if (s == 2)
    hipLaunchKernelGGL((bp_bwd<2>), grid, dim3(NT), 0, st, a);
  else if (s == 3)
    hipLaunchKernelGGL((bp_bwd<3>), grid, dim3(NT), 0, st, a);
  else
    hipLaunchKernelGGL((bp_bwd<4>), grid, dim3(NT), 0, st, a);
}

}  // namespace bp
}  // namespace ssg

using namespace ssg::bp;

extern "C" {

size_t ssg_bp_workspace_bytes(int planes, int H, int W, int s) {
  if (check_shape(planes, H, W, s)) return 0;
  Args a{};
  geometry(a, planes, H, W, s);
  return layout(a).total;
}

int ssg_bp_downsample(const float *x, int planes, int H, int W, int s, float *y_out, ssg_stream_t stream) {
  if (!x || !y_out) return SSG_E_BADARG;
  const int rc = check_shape(planes, H, W, s);
  if (rc) return rc;
  Args a{};
  geometry(a, planes, H, W, s);
  a.x = x;
  a.y = y_out;
  launch_fwd(a, s, (hipStream_t)stream);
  return (int)hipGetLastError();
}

int ssg_bp_downsample_backward(const float *grad_y, int planes, int H, int W, int s, float *grad_x,
                               ssg_stream_t stream) {
  if (!grad_y || !grad_x) return SSG_E_BADARG;
  const int rc = check_shape(planes, H, W, s);
  if (rc) return rc;
  Args a{};
  geometry(a, planes, H, W, s);
  a.gy = grad_y;
  a.grad = grad_x;
  a.scale = 1.f;
  launch_bwd(a, s, (hipStream_t)stream);
  return (int)hipGetLastError();
}

int ssg_bp_loss(const float *x, const float *lq, int planes, int H, int W, int s, float loss_weight, int mean,
                float *loss_out, float *grad_x, float *y_out, void *workspace, size_t workspace_bytes,
                ssg_stream_t stream) {
  if (!x || !lq || !loss_out || !workspace || loss_weight != loss_weight) return SSG_E_BADARG;
  const int rc = check_shape(planes, H, W, s);
  if (rc) return rc;
  Args a{};
  geometry(a, planes, H, W, s);
  const Layout L = layout(a);
  const int ws_rc = check_workspace(workspace, workspace_bytes, L.total);
  if (ws_rc) return ws_rc;
  a.x = x;
  a.lq = lq;
  a.y = y_out;
  a.sg = grad_x ? (float *)((char *)workspace + L.sg) : nullptr;
  a.part = (double *)((char *)workspace + L.part);
  a.gy = a.sg;
  a.grad = grad_x;
  a.loss = loss_out;
  a.loss_scale = mean ? (double)loss_weight / ((double)planes * a.ho * a.wo) : (double)loss_weight;
  a.scale = (float)a.loss_scale;
  launch_fwd(a, s, (hipStream_t)stream);
  launch_bwd(a, s, (hipStream_t)stream);
  return (int)hipGetLastError();
}

}  // extern "C"
