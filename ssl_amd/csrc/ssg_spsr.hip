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
//   sums       every fp32 l is widened and ADDED IN FP64: a thread adds its elements in index order, a wave folds by the
//              shuffle tree, a workgroup adds its four waves in order, one workgroup folds the partials (thread i takes
//              i, i + 256, ..., then an LDS tree).  No atomics: the same bits from call to call.
//   gradients  grad[i] = (float)(coef[0] (double)l'(d_i)), coef one double on the device (upstream x weight / n).
// Every kernel walks the flat index space in groups of four behind x's first 16-byte boundary (scalar head and tail), 256
// threads, one group per thread and trip, at most MAX_WG workgroups, grid-stride beyond.  An element's (row, column)
// comes from its own flat index, so a group may straddle a row or a plane and W need not be a multiple of 4.  Any other
// tensor of a call is accessed 16 bytes wide where it shares x's alignment and element by element where it does not.
// The forward kernels take the group's own four values in one load (they are the horizontal neighbours of each other) and
// the rows above and below in one load each where W is a multiple of 4 and the group lies in one row; the gather
// kernels read their distance-2 neighbourhood element by element from L1 / L2 (lanes are consecutive: coalesced).
// A plane's results do not depend on the planes around it: plane p of a batch is the same bits as the plane alone.
// The launchers trust their arguments: the entry points in ssg_api.hip refuse bad ones before any launch.
#include <math.h>

#include "ssg_host.hpp"

namespace ssg {
namespace spsr {

constexpr int NT = 256;        // threads per workgroup
constexpr int EPT = 4;         // elements per thread and trip
constexpr int MAX_WG = 1024;   // the grid cap (ssg_spsr_grid_cap): four workgroups per CU
constexpr float MAP_EPS = 1e-6f;

struct Planes {
  unsigned H, W;
  size_t n;
};

// l and l' of one difference
template <int KIND>
__device__ __forceinline__ float crit(float d, float eps) {
  if (KIND == SSG_PIX_L1) return fabsf(d);
  if (KIND == SSG_PIX_MSE) return d * d;
  return sqrtf(d * d + eps);
}

template <int KIND>
__device__ __forceinline__ float dcrit(float d, float eps) {
  if (KIND == SSG_PIX_L1) return d > 0.f ? 1.f : (d < 0.f ? -1.f : d * 0.f);   // (0 for +-0, NaN for a NaN)
  if (KIND == SSG_PIX_MSE) return 2.f * d;
  return d / sqrtf(d * d + eps);
}

__device__ __forceinline__ size_t head_of(const float *x, size_t n) {
  const size_t h = ((16 - ((size_t)x & 15)) & 15) / sizeof(float);
  return h < n ? h : n;
}

__device__ __forceinline__ bool wide(const float *p, size_t head) { return (((size_t)(p + head)) & 15) == 0; }

__device__ __forceinline__ void load4(const float *p, bool vec, float o[4]) {
  if (vec) {
    const float4 v = *(const float4 *)p;
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
  } else {
    o[0] = p[0], o[1] = p[1], o[2] = p[2], o[3] = p[3];
  }
}

__device__ __forceinline__ void store4(float *p, bool vec, const float o[4]) {
  if (vec) {
    *(float4 *)p = make_float4(o[0], o[1], o[2], o[3]);
  } else {
    p[0] = o[0], p[1] = o[1], p[2] = o[2], p[3] = o[3];
  }
}

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

// one fp64 partial per workgroup
__device__ __forceinline__ void fold_workgroup(double L, double *part) {
  __shared__ double w0[NT / 64];
  for (int o = 32; o > 0; o >>= 1) L += __shfl_down(L, o, 64);
  if ((threadIdx.x & 63) == 0) w0[threadIdx.x >> 6] = L;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (w0[0] + w0[1]) + (w0[2] + w0[3]);
}

__global__ __launch_bounds__(NT) void spsr_fold_kernel(const double *part, int nparts, double *out) {
  __shared__ double s0[NT];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += NT) a += part[i];
  s0[threadIdx.x] = a;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s0[threadIdx.x] += s0[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s0[0];
}

// the flat walk every kernel shares: ONE(idx) for an element of the head or the tail, QUAD(idx) for a group
#define SSG_SPSR_WALK(PTR_, CNT_, ONE_, QUAD_)                                                          \
  {                                                                                                     \
    const size_t w_head = head_of(PTR_, CNT_), w_n4 = (CNT_ - w_head) / EPT;                            \
    const size_t w_first = (size_t)blockIdx.x * NT + threadIdx.x, w_stride = (size_t)gridDim.x * NT;    \
    for (size_t w_e = w_first; w_e < w_head; w_e += w_stride) { ONE_(w_e) }                             \
    for (size_t w_q = w_first; w_q < w_n4; w_q += w_stride) { QUAD_((w_head + EPT * w_q)) }             \
    for (size_t w_e = w_head + EPT * w_n4 + w_first; w_e < CNT_; w_e += w_stride) { ONE_(w_e) }         \
  }

// ---- the map ----
__global__ __launch_bounds__(NT) void spsr_map_kernel(const float *x, Planes g, float *map) {
  const bool mv = wide(map, head_of(x, g.n));
#define ONE(e) map[e] = map_one(x, g, e);
#define QUAD(e)          \
  float m[4];            \
  map_quad(x, g, e, m);  \
  store4(map + e, mv, m);
  SSG_SPSR_WALK(x, g.n, ONE, QUAD)
#undef ONE
#undef QUAD
}

// ---- crit(G(x), G(t)) summed, G(x) optionally written ----
template <int KIND>
__global__ __launch_bounds__(NT) void spsr_loss_kernel(const float *x, const float *t, Planes g, float eps, float *map,
                                                       double *part) {
  const size_t hd = head_of(x, g.n);
  const bool tv = wide(t, hd), mv = map && wide(map, hd);
  double L = 0.0;
#define ONE(e)                                \
  const float mx = map_one(x, g, e);          \
  if (map) map[e] = mx;                       \
  L += (double)crit<KIND>(mx - map_one(t, g, e), eps);
#define QUAD(e)                                                                      \
  float mx[4], mt[4];                                                                \
  map_quad(x, g, e, mx);                                                             \
  if (tv) {                                                                          \
    map_quad(t, g, e, mt);                                                           \
  } else {                                                                           \
    for (int k = 0; k < 4; ++k) mt[k] = map_one(t, g, e + k);                        \
  }                                                                                  \
  if (map) store4(map + e, mv, mx);                                                  \
  for (int k = 0; k < 4; ++k) L += (double)crit<KIND>(mx[k] - mt[k], eps);
  SSG_SPSR_WALK(x, g.n, ONE, QUAD)
#undef ONE
#undef QUAD
  fold_workgroup(L, part);
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
#define ONE(e) L += (double)crit<KIND>(branch[e] - map_one(gt, g, e), eps);
#define QUAD(e)                \
  float m[4], p[4];            \
  map_quad(gt, g, e, m);       \
  load4(branch + e, bv, p);    \
  for (int k = 0; k < 4; ++k) L += (double)crit<KIND>(p[k] - m[k], eps);
  SSG_SPSR_WALK(gt, g.n, ONE, QUAD)
#undef ONE
#undef QUAD
  fold_workgroup(L, part);
}

template <int KIND>
__global__ __launch_bounds__(NT) void spsr_branch_grad_kernel(const float *branch, const float *gt, Planes g, float eps,
                                                              const double *coef, float *grad) {
  const size_t hd = head_of(gt, g.n);
  const bool bv = wide(branch, hd), gv = wide(grad, hd);
  const double c = coef[0];
#define ONE(e) grad[e] = (float)(c * (double)dcrit<KIND>(branch[e] - map_one(gt, g, e), eps));
#define QUAD(e)                                                                               \
  float m[4], p[4], r[4];                                                                     \
  map_quad(gt, g, e, m);                                                                      \
  load4(branch + e, bv, p);                                                                   \
  for (int k = 0; k < 4; ++k) r[k] = (float)(c * (double)dcrit<KIND>(p[k] - m[k], eps));      \
  store4(grad + e, gv, r);
  SSG_SPSR_WALK(gt, g.n, ONE, QUAD)
#undef ONE
#undef QUAD
}

// ---- the streaming pixel criteria on two flat tensors ----
template <int KIND>
__global__ __launch_bounds__(NT) void pixel_sums_kernel(const float *a, const float *b, size_t n, float eps,
                                                        double *part) {
  const bool bv = wide(b, head_of(a, n));
  double L = 0.0;
#define ONE(e) L += (double)crit<KIND>(a[e] - b[e], eps);
#define QUAD(e)           \
  float p[4], q[4];       \
  load4(a + e, true, p);  \
  load4(b + e, bv, q);    \
  for (int k = 0; k < 4; ++k) L += (double)crit<KIND>(p[k] - q[k], eps);
  SSG_SPSR_WALK(a, n, ONE, QUAD)
#undef ONE
#undef QUAD
  fold_workgroup(L, part);
}

template <int KIND>
__global__ __launch_bounds__(NT) void pixel_grad_kernel(const float *a, const float *b, size_t n, float eps,
                                                        const double *coef, float *grad) {
  const size_t hd = head_of(a, n);
  const bool bv = wide(b, hd), gv = wide(grad, hd);
  const double c = coef[0];
#define ONE(e) grad[e] = (float)(c * (double)dcrit<KIND>(a[e] - b[e], eps));
#define QUAD(e)                                                                           \
  float p[4], q[4], r[4];                                                                 \
  load4(a + e, true, p);                                                                  \
  load4(b + e, bv, q);                                                                    \
  for (int k = 0; k < 4; ++k) r[k] = (float)(c * (double)dcrit<KIND>(p[k] - q[k], eps));  \
  store4(grad + e, gv, r);
  SSG_SPSR_WALK(a, n, ONE, QUAD)
#undef ONE
#undef QUAD
}

#undef SSG_SPSR_WALK

inline unsigned grid_for(size_t n, int per_thread) {
  const size_t per = (size_t)NT * per_thread, want = (n + per - 1) / per;
  return (unsigned)(want < 1 ? 1 : (want > MAX_WG ? MAX_WG : want));
}

// the partials' fold behind a sums kernel (a single workgroup has written sum_out itself)
inline int finish_sums(unsigned grid, const double *part, double *sum_out, hipStream_t st) {
  if (grid > 1) hipLaunchKernelGGL(spsr_fold_kernel, dim3(1), dim3(NT), 0, st, part, (int)grid, sum_out);
  return (int)hipGetLastError();
}

}  // namespace spsr

int spsr_grid_cap() { return spsr::MAX_WG; }

size_t spsr_workspace_bytes() { return sizeof(double) * spsr::MAX_WG; }

#define SSG_SPSR_KINDS(CALL)                            \
  switch (kind) {                                       \
    case SSG_PIX_L1: CALL(SSG_PIX_L1); break;           \
    case SSG_PIX_MSE: CALL(SSG_PIX_MSE); break;         \
    default: CALL(SSG_PIX_CHARBONNIER); break;          \
  }

int launch_spsr_map(const float *x, int planes, int H, int W, float *map, hipStream_t st) {
  using namespace spsr;
  const Planes g{(unsigned)H, (unsigned)W, (size_t)planes * H * W};
  hipLaunchKernelGGL(spsr_map_kernel, dim3(grid_for(g.n, EPT)), dim3(NT), 0, st, x, g, map);
  return (int)hipGetLastError();
}

int launch_spsr_loss(const float *x, const float *t, int planes, int H, int W, int kind, float eps, float *map_out,
                     void *workspace, double *sum_out, hipStream_t st) {
  using namespace spsr;
  const Planes g{(unsigned)H, (unsigned)W, (size_t)planes * H * W};
  const unsigned grid = grid_for(g.n, EPT);
  double *part = grid == 1 ? sum_out : (double *)workspace;
#define CALL(K) hipLaunchKernelGGL(spsr_loss_kernel<K>, dim3(grid), dim3(NT), 0, st, x, t, g, eps, map_out, part)
  SSG_SPSR_KINDS(CALL)
#undef CALL
  return finish_sums(grid, part, sum_out, st);
}

int launch_spsr_gather(const float *x, const float *t, const float *gmap, const double *coef, int planes, int H, int W,
                       int kind, float eps, float *dx, hipStream_t st) {
  using namespace spsr;
  const bool loss = t != nullptr;
  const Planes g{(unsigned)H, (unsigned)W, (size_t)planes * H * W};
  const unsigned grid = grid_for(g.n, 1);
  if (!loss) {
    hipLaunchKernelGGL((spsr_gather_kernel<SSG_PIX_L1, false>), dim3(grid), dim3(NT), 0, st, x, t, gmap, coef, g, eps, dx);
  } else {
#define CALL(K) hipLaunchKernelGGL((spsr_gather_kernel<K, true>), dim3(grid), dim3(NT), 0, st, x, t, gmap, coef, g, eps, dx)
    SSG_SPSR_KINDS(CALL)
#undef CALL
  }
  return (int)hipGetLastError();
}

int launch_spsr_branch_sums(const float *branch, const float *gt, int planes, int H, int W, int kind, float eps,
                            void *workspace, double *sum_out, hipStream_t st) {
  using namespace spsr;
  const Planes g{(unsigned)H, (unsigned)W, (size_t)planes * H * W};
  const unsigned grid = grid_for(g.n, EPT);
  double *part = grid == 1 ? sum_out : (double *)workspace;
#define CALL(K) hipLaunchKernelGGL(spsr_branch_sums_kernel<K>, dim3(grid), dim3(NT), 0, st, branch, gt, g, eps, part)
  SSG_SPSR_KINDS(CALL)
#undef CALL
  return finish_sums(grid, part, sum_out, st);
}

int launch_spsr_branch_grad(const float *branch, const float *gt, int planes, int H, int W, int kind, float eps,
                            const double *coef, float *grad, hipStream_t st) {
  using namespace spsr;
  const Planes g{(unsigned)H, (unsigned)W, (size_t)planes * H * W};
#define CALL(K) \
  hipLaunchKernelGGL(spsr_branch_grad_kernel<K>, dim3(grid_for(g.n, EPT)), dim3(NT), 0, st, branch, gt, g, eps, coef, grad)
  SSG_SPSR_KINDS(CALL)
#undef CALL
  return (int)hipGetLastError();
}

int launch_pixel_sums(const float *a, const float *b, size_t n, int kind, float eps, void *workspace, double *sum_out,
                      hipStream_t st) {
  using namespace spsr;
  const unsigned grid = grid_for(n, EPT);
  double *part = grid == 1 ? sum_out : (double *)workspace;
#define CALL(K) hipLaunchKernelGGL(pixel_sums_kernel<K>, dim3(grid), dim3(NT), 0, st, a, b, n, eps, part)
  SSG_SPSR_KINDS(CALL)
#undef CALL
  return finish_sums(grid, part, sum_out, st);
}

int launch_pixel_grad(const float *a, const float *b, size_t n, int kind, float eps, const double *coef, float *grad,
                      hipStream_t st) {
  using namespace spsr;
#define CALL(K) hipLaunchKernelGGL(pixel_grad_kernel<K>, dim3(grid_for(n, EPT)), dim3(NT), 0, st, a, b, n, eps, coef, grad)
  SSG_SPSR_KINDS(CALL)
#undef CALL
  return (int)hipGetLastError();
}

#undef SSG_SPSR_KINDS

}  // namespace ssg
