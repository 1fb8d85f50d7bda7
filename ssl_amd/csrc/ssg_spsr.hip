// SPSR's gradient map and the pixel criteria on it: basicsr/models/spsrssl_model.py:18-84 (Get_gradient and
// Get_gradient_nopadding, the same arithmetic), :363 cri_pix_gradSR(G(output), G(gt)), :368 cri_pix_gradBranch(branch,
// G(gt)), and basicsr/losses/basic_loss.py:69-128 (MSELoss, CharbonnierLoss).  fp32 NCHW contiguous; a batch is
// planes = B C independent H x W planes, any planes, H, W >= 1 with planes H W < 2^31.
//
// Contract (this file is compiled with -ffp-contract=off; every operation is fp32 and rounded on its own).
//   map        v = x[i+1,j] - x[i-1,j],  h = x[i,j+1] - x[i,j-1]  (a neighbour outside the plane is 0 and is never read:
//              a plane never reads its neighbour plane's rows),  m = sqrtf((v v + h h) + 1e-6f)
//   adjoint    dx[i,j] = ((a[i-1,j] - a[i+1,j]) + b[i,j-1]) - b[i,j+1],  a = (w v) / m,  b = (w h) / m at the neighbour,
//              recomputed from x (distance 2); a term whose element lies outside the plane is 0.  w is the gradient that
//              arrives at the map value: g_map for the map's own backward,
//              (float)(coef[0] (double)crit'(m_x - m_t)) [+ g_map] for the fused loss.
//   criteria   d = p - q (one subtraction)
//              SSG_PIX_L1           l = |d|                 l' = 1, -1 or 0 (d = 0), NaN for a NaN
//              SSG_PIX_MSE          l = d d                 l' = 2 d
//              SSG_PIX_CHARBONNIER  l = sqrtf(d d + eps)    l' = d / sqrtf(d d + eps)
//   sums       every fp32 l is widened and added in fp64 in the fixed order of ssg_stream.hpp: the same bits from call
//              to call.
//   gradients  grad[i] = (float)(coef[0] (double)l'(d_i)), coef one double on the device (upstream x weight / n).
// Every kernel but the gather walks the flat index space with ssg_stream.hpp's walk and launch geometry.  An element's
// (row, column) comes from its own flat index, so a group may straddle a row or a plane and W need not be a multiple
// of 4.  Any other tensor of a call is accessed 16 bytes wide where it shares x's alignment, element by element otherwise.
// The forward kernels take the group's own four values in one load (they are the horizontal neighbours of each other) and
// the rows above and below in one load each where W is a multiple of 4 and the group lies in one row; the gather
// kernels read their distance-2 neighbourhood element by element from L1 / L2 (lanes are consecutive: coalesced).
// A plane's results do not depend on the planes around it: plane p of a batch is the same bits as the plane alone.
// This file defines the entry points ssg_spsr_* (eight) and ssg_pixel_sums / ssg_pixel_grad, at its end: they refuse bad
// arguments before any launch.
#include "ssg_stream.hpp"

namespace ssg {
namespace spsr {

using namespace stream;

constexpr float MAP_EPS = 1e-6f;

struct Planes {
  unsigned H, W;
  size_t n;
};

// (l and l' of one difference, crit<KIND> and dcrit<KIND>, are ssg_stream.hpp's: ssg_mcrit.hip uses the same two)

// (row in its plane, column) of a flat index
__device__ __forceinline__ void place(const Planes &g, size_t idx, unsigned &i, unsigned &j) {
  const unsigned row = (unsigned)idx / g.W;
  j = (unsigned)idx - row * g.W;
  i = row % g.H;
}

__device__ __forceinline__ float map_of(float v, float h) { return sqrtf((v * v + h * h) + MAP_EPS); }

// v, h, m of the element (i, j) at flat index idx, its four neighbours read one by one
__device__ __forceinline__ float map_at(const float *x, const Planes &g, size_t idx, unsigned i, unsigned j, float &v,
                                        float &h) {
  const float up = i > 0 ? x[idx - g.W] : 0.f, dn = i + 1 < g.H ? x[idx + g.W] : 0.f;
  const float lf = j > 0 ? x[idx - 1] : 0.f, rt = j + 1 < g.W ? x[idx + 1] : 0.f;
  v = dn - up;
  h = rt - lf;
  return map_of(v, h);
}

// the map of the four elements idx .. idx + 3, all inside [0, n); x + idx is 16-byte aligned
__device__ __forceinline__ void map_quad(const float *x, const Planes &g, size_t idx, float m[4]) {
  unsigned i, j;
  place(g, idx, i, j);
  float c[4];
  load4(x + idx, true, c);
  if (j + 3 < g.W && (g.W & 3) == 0) {   // one row, and the rows above and below are aligned like this one
    float up[4] = {0.f, 0.f, 0.f, 0.f}, dn[4] = {0.f, 0.f, 0.f, 0.f};
    if (i > 0) load4(x + idx - g.W, true, up);
    if (i + 1 < g.H) load4(x + idx + g.W, true, dn);
    const float lf = j > 0 ? x[idx - 1] : 0.f, rt = j + 4 < g.W ? x[idx + 4] : 0.f;
    m[0] = map_of(dn[0] - up[0], c[1] - lf);
    m[1] = map_of(dn[1] - up[1], c[2] - c[0]);
    m[2] = map_of(dn[2] - up[2], c[3] - c[1]);
    m[3] = map_of(dn[3] - up[3], rt - c[2]);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float up = i > 0 ? x[idx + k - g.W] : 0.f, dn = i + 1 < g.H ? x[idx + k + g.W] : 0.f;
    const float lf = j > 0 ? (k > 0 ? c[k - 1] : x[idx - 1]) : 0.f;
    const float rt = j + 1 < g.W ? (k < 3 ? c[k + 1] : x[idx + 4]) : 0.f;
    m[k] = map_of(dn - up, rt - lf);
    if (++j == g.W) {
      j = 0;
      if (++i == g.H) i = 0;
    }
  }
}

__device__ __forceinline__ float map_one(const float *x, const Planes &g, size_t idx) {
  unsigned i, j;
  place(g, idx, i, j);
  float v, h;
  return map_at(x, g, idx, i, j, v, h);
}

// ---- the map ----
__global__ __launch_bounds__(NT) void spsr_map_kernel(const float *x, Planes g, float *map) {
  const bool mv = wide(map, head_of(x, g.n));
  walk(
      x, g.n, [&](size_t e) { map[e] = map_one(x, g, e); },
      [&](size_t e) {
        float m[4];
        map_quad(x, g, e, m);
        store4(map + e, mv, m);
      });
}

// ---- crit(G(x), G(t)) summed, G(x) optionally written ----
template <int KIND>
__global__ __launch_bounds__(NT) void spsr_loss_kernel(const float *x, const float *t, Planes g, float eps, float *map,
                                                       double *part) {
  const size_t hd = head_of(x, g.n);
  const bool tv = wide(t, hd), mv = map && wide(map, hd);
  double L = 0.0;
  walk(
      x, g.n,
      [&](size_t e) {
        const float mx = map_one(x, g, e);
        if (map) map[e] = mx;
        L += (double)crit<KIND>(mx - map_one(t, g, e), eps);
      },
      [&](size_t e) {
        float mx[4], mt[4];
        map_quad(x, g, e, mx);
        if (tv) {
          map_quad(t, g, e, mt);
        } else {
          for (int k = 0; k < 4; ++k) mt[k] = map_one(t, g, e + k);
        }
        if (map) store4(map + e, mv, mx);
        for (int k = 0; k < 4; ++k) L += (double)crit<KIND>(mx[k] - mt[k], eps);
      });
  workgroup_partials<1>({L}, part);
}

// ---- the gather: the map's adjoint, with the weight that arrives at each map value formed on the way ----
// LOSS: w = (float)(coef[0] crit'(m_x - m_t)); gmap (nullable when LOSS) is added to it, or is w itself.
template <int KIND, bool LOSS>
__device__ __forceinline__ void gather_term(const float *x, const float *t, const float *gmap, const Planes &g, size_t idx,
                                            unsigned i, unsigned j, double c, float eps, float &a, float &b) {
  float v, h;
  const float m = map_at(x, g, idx, i, j, v, h);
  float w;
  if (LOSS) {
    float tv, th;
    w = (float)(c * (double)dcrit<KIND>(m - map_at(t, g, idx, i, j, tv, th), eps));
    if (gmap) w = w + gmap[idx];
  } else {
    w = gmap[idx];
  }
  a = (w * v) / m;
  b = (w * h) / m;
}

template <int KIND, bool LOSS>
__global__ __launch_bounds__(NT) void spsr_gather_kernel(const float *x, const float *t, const float *gmap,
                                                         const double *coef, Planes g, float eps, float *dx) {
  const double c = LOSS ? coef[0] : 0.0;
  const size_t first = (size_t)blockIdx.x * NT + threadIdx.x, stride = (size_t)gridDim.x * NT;
  for (size_t idx = first; idx < g.n; idx += stride) {
    unsigned i, j;
    place(g, idx, i, j);
    float au = 0.f, ad = 0.f, bl = 0.f, br = 0.f, o;
    if (i > 0) gather_term<KIND, LOSS>(x, t, gmap, g, idx - g.W, i - 1, j, c, eps, au, o);
    if (i + 1 < g.H) gather_term<KIND, LOSS>(x, t, gmap, g, idx + g.W, i + 1, j, c, eps, ad, o);
    if (j > 0) gather_term<KIND, LOSS>(x, t, gmap, g, idx - 1, i, j - 1, c, eps, o, bl);
    if (j + 1 < g.W) gather_term<KIND, LOSS>(x, t, gmap, g, idx + 1, i, j + 1, c, eps, o, br);
    dx[idx] = ((au - ad) + bl) - br;
  }
}

// ---- crit(branch, G(gt)): the walk is gt's, whose map is formed on the fly ----
template <int KIND>
__global__ __launch_bounds__(NT) void spsr_branch_sums_kernel(const float *branch, const float *gt, Planes g, float eps,
                                                              double *part) {
  const bool bv = wide(branch, head_of(gt, g.n));
  double L = 0.0;
  walk(
      gt, g.n, [&](size_t e) { L += (double)crit<KIND>(branch[e] - map_one(gt, g, e), eps); },
      [&](size_t e) {
        float m[4], p[4];
        map_quad(gt, g, e, m);
        load4(branch + e, bv, p);
        for (int k = 0; k < 4; ++k) L += (double)crit<KIND>(p[k] - m[k], eps);
      });
  workgroup_partials<1>({L}, part);
}

template <int KIND>
__global__ __launch_bounds__(NT) void spsr_branch_grad_kernel(const float *branch, const float *gt, Planes g, float eps,
                                                              const double *coef, float *grad) {
  const size_t hd = head_of(gt, g.n);
  const bool bv = wide(branch, hd), gv = wide(grad, hd);
  const double c = coef[0];
  walk(
      gt, g.n, [&](size_t e) { grad[e] = (float)(c * (double)dcrit<KIND>(branch[e] - map_one(gt, g, e), eps)); },
      [&](size_t e) {
        float m[4], p[4], r[4];
        map_quad(gt, g, e, m);
        load4(branch + e, bv, p);
        for (int k = 0; k < 4; ++k) r[k] = (float)(c * (double)dcrit<KIND>(p[k] - m[k], eps));
        store4(grad + e, gv, r);
      });
}

// ---- the streaming pixel criteria on two flat tensors ----
template <int KIND>
__global__ __launch_bounds__(NT) void pixel_sums_kernel(const float *a, const float *b, size_t n, float eps,
                                                        double *part) {
  const bool bv = wide(b, head_of(a, n));
  double L = 0.0;
  walk(
      a, n, [&](size_t e) { L += (double)crit<KIND>(a[e] - b[e], eps); },
      [&](size_t e) {
        float p[4], q[4];
        load4(a + e, true, p);
        load4(b + e, bv, q);
        for (int k = 0; k < 4; ++k) L += (double)crit<KIND>(p[k] - q[k], eps);
      });
  workgroup_partials<1>({L}, part);
}

template <int KIND>
__global__ __launch_bounds__(NT) void pixel_grad_kernel(const float *a, const float *b, size_t n, float eps,
                                                        const double *coef, float *grad) {
  const size_t hd = head_of(a, n);
  const bool bv = wide(b, hd), gv = wide(grad, hd);
  const double c = coef[0];
  walk(
      a, n, [&](size_t e) { grad[e] = (float)(c * (double)dcrit<KIND>(a[e] - b[e], eps)); },
      [&](size_t e) {
        float p[4], q[4], r[4];
        load4(a + e, true, p);
        load4(b + e, bv, q);
        for (int k = 0; k < 4; ++k) r[k] = (float)(c * (double)dcrit<KIND>(p[k] - q[k], eps));
        store4(grad + e, gv, r);
      });
}

inline Planes planes_of(int planes, int H, int W) { return Planes{(unsigned)H, (unsigned)W, (size_t)planes * H * W}; }

static int check_planes(int planes, int H, int W) {
  if (planes < 1 || H < 1 || W < 1) return SSG_E_BADARG;
  return (unsigned long long)planes * (unsigned long long)H * (unsigned long long)W >= (1ull << 31) ? SSG_E_BADARG : 0;
}

static int check_kind(int kind, float eps) {
  if (kind < SSG_PIX_L1 || kind > SSG_PIX_CHARBONNIER) return SSG_E_BADARG;
  return eps >= 0.f && eps <= 3.402823466e38f ? 0 : SSG_E_BADARG;   // (a NaN fails both comparisons)
}

// (file-local and in front of launch_gather, which has two callers: the order in which this file first names its kernel
// templates is the order of the kernels in the code object)
static int launch_loss(const float *x, const float *t, int planes, int H, int W, int kind, float eps, float *map_out,
                       void *workspace, double *sum_out, hipStream_t st) {
  const Planes g = planes_of(planes, H, W);
  const unsigned grid = grid_for(g.n, EPT);
  double *part = partials_of(grid, workspace, sum_out);
  with_pixel_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(spsr_loss_kernel<decltype(k)::value>, dim3(grid), dim3(NT), 0, st, x, t, g, eps, map_out, part);
  });
  return finish_sums<1>(grid, part, sum_out, st);
}

// t == nullptr: the map's own adjoint of gmap; else the fused loss's, coef[0] crit' (+ gmap where given)
static int launch_gather(const float *x, const float *t, const float *gmap, const double *coef, int planes, int H, int W,
                         int kind, float eps, float *dx, hipStream_t st) {
  const Planes g = planes_of(planes, H, W);
  const unsigned grid = grid_for(g.n, 1);
  if (!t) {
    hipLaunchKernelGGL((spsr_gather_kernel<SSG_PIX_L1, false>), dim3(grid), dim3(NT), 0, st, x, t, gmap, coef, g, eps, dx);
  } else {
    with_pixel_kind(kind, [&](auto k) {
      hipLaunchKernelGGL((spsr_gather_kernel<decltype(k)::value, true>), dim3(grid), dim3(NT), 0, st, x, t, gmap, coef, g,
                         eps, dx);
    });
  }
  return (int)hipGetLastError();
}

}  // namespace spsr

}  // namespace ssg

// ---- (R) the entry points: every refusal is decided here, before the launch ----
using namespace ssg;
using namespace ssg::spsr;

extern "C" {

size_t ssg_spsr_workspace_bytes(void) { return sizeof(double) * MAX_WG; }

int ssg_spsr_grid_cap(void) { return MAX_WG; }

int ssg_spsr_map(const float *x, int planes, int H, int W, float *map, ssg_stream_t stream) {
  if (!x || !map) return SSG_E_BADARG;
  if (const int rc = check_planes(planes, H, W)) return rc;
  if (unaligned(x, 4) || unaligned(map, 4)) return SSG_E_ALIGN;
  const Planes g = planes_of(planes, H, W);
  hipLaunchKernelGGL(spsr_map_kernel, dim3(grid_for(g.n, EPT)), dim3(NT), 0, (hipStream_t)stream, x, g, map);
  return (int)hipGetLastError();
}

int ssg_spsr_map_backward(const float *x, const float *grad_map, int planes, int H, int W, float *grad_x,
                          ssg_stream_t stream) {
  if (!x || !grad_map || !grad_x) return SSG_E_BADARG;
  if (const int rc = check_planes(planes, H, W)) return rc;
  if (unaligned(x, 4) || unaligned(grad_map, 4) || unaligned(grad_x, 4)) return SSG_E_ALIGN;
  return launch_gather(x, nullptr, grad_map, nullptr, planes, H, W, SSG_PIX_L1, 0.f, grad_x, (hipStream_t)stream);
}

int ssg_spsr_loss(const float *x, const float *target, int planes, int H, int W, int kind, float eps, float *map_out,
                  void *workspace, double *sum_out, ssg_stream_t stream) {
  if (!x || !target || !workspace || !sum_out) return SSG_E_BADARG;
  if (const int rc = check_planes(planes, H, W)) return rc;
  if (const int rc = check_kind(kind, eps)) return rc;
  if (unaligned(x, 4) || unaligned(target, 4) || unaligned(map_out, 4) || unaligned(workspace, 8) ||
      unaligned(sum_out, 8))
    return SSG_E_ALIGN;
  return launch_loss(x, target, planes, H, W, kind, eps, map_out, workspace, sum_out, (hipStream_t)stream);
}

int ssg_spsr_loss_backward(const float *x, const float *target, const float *grad_map, const double *coef, int planes,
                           int H, int W, int kind, float eps, float *grad_x, ssg_stream_t stream) {
  if (!x || !target || !coef || !grad_x) return SSG_E_BADARG;
  if (const int rc = check_planes(planes, H, W)) return rc;
  if (const int rc = check_kind(kind, eps)) return rc;
  if (unaligned(x, 4) || unaligned(target, 4) || unaligned(grad_map, 4) || unaligned(grad_x, 4) ||
      unaligned(coef, 8))
    return SSG_E_ALIGN;
  return launch_gather(x, target, grad_map, coef, planes, H, W, kind, eps, grad_x, (hipStream_t)stream);
}

int ssg_spsr_branch_loss(const float *branch, const float *gt, int planes, int H, int W, int kind, float eps,
                         void *workspace, double *sum_out, ssg_stream_t stream) {
  if (!branch || !gt || !workspace || !sum_out) return SSG_E_BADARG;
  if (const int rc = check_planes(planes, H, W)) return rc;
  if (const int rc = check_kind(kind, eps)) return rc;
  if (unaligned(branch, 4) || unaligned(gt, 4) || unaligned(workspace, 8) || unaligned(sum_out, 8))
    return SSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const Planes g = planes_of(planes, H, W);
  const unsigned grid = grid_for(g.n, EPT);
  double *part = partials_of(grid, workspace, sum_out);
  with_pixel_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(spsr_branch_sums_kernel<decltype(k)::value>, dim3(grid), dim3(NT), 0, st, branch, gt, g, eps, part);
  });
  return finish_sums<1>(grid, part, sum_out, st);
}

int ssg_spsr_branch_grad(const float *branch, const float *gt, int planes, int H, int W, int kind, float eps,
                         const double *coef, float *grad_branch, ssg_stream_t stream) {
  if (!branch || !gt || !coef || !grad_branch) return SSG_E_BADARG;
  if (const int rc = check_planes(planes, H, W)) return rc;
  if (const int rc = check_kind(kind, eps)) return rc;
  if (unaligned(branch, 4) || unaligned(gt, 4) || unaligned(grad_branch, 4) || unaligned(coef, 8))
    return SSG_E_ALIGN;
  const Planes g = planes_of(planes, H, W);
  with_pixel_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(spsr_branch_grad_kernel<decltype(k)::value>, dim3(grid_for(g.n, EPT)), dim3(NT), 0,
                       (hipStream_t)stream, branch, gt, g, eps, coef, grad_branch);
  });
  return (int)hipGetLastError();
}

int ssg_pixel_sums(const float *pred, const float *target, size_t n, int kind, float eps, void *workspace,
                   double *sum_out, ssg_stream_t stream) {
  if (!pred || !target || !workspace || !sum_out || n < 1) return SSG_E_BADARG;
  if (const int rc = check_kind(kind, eps)) return rc;
  if (unaligned(pred, 4) || unaligned(target, 4) || unaligned(workspace, 8) || unaligned(sum_out, 8))
    return SSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(n, EPT);
  double *part = partials_of(grid, workspace, sum_out);
  with_pixel_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(pixel_sums_kernel<decltype(k)::value>, dim3(grid), dim3(NT), 0, st, pred, target, n, eps, part);
  });
  return finish_sums<1>(grid, part, sum_out, st);
}

int ssg_pixel_grad(const float *pred, const float *target, size_t n, int kind, float eps, const double *coef,
                   float *grad_pred, ssg_stream_t stream) {
  if (!pred || !target || !coef || !grad_pred || n < 1) return SSG_E_BADARG;
  if (const int rc = check_kind(kind, eps)) return rc;
  if (unaligned(pred, 4) || unaligned(target, 4) || unaligned(grad_pred, 4) || unaligned(coef, 8))
    return SSG_E_ALIGN;
  with_pixel_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(pixel_grad_kernel<decltype(k)::value>, dim3(grid_for(n, EPT)), dim3(NT), 0, (hipStream_t)stream,
                       pred, target, n, eps, coef, grad_pred);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
