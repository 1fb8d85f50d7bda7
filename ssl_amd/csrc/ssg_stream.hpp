// What the streaming criteria share (ssg_gan.hip, ssg_spsr.hip, ssg_mcrit.hip, and the partial sums of ssg_grow.hip's L1 / KL criteria):
// the launch geometry, the walk over a flat fp32 tensor, the fixed-order fp64 sum and the fold of its partials.  One
// definition each: a fix to the head / tail split or to the order of the sum reaches every file.
//
// Contract, for every kernel built on this header.
//   walk    256 threads, 16-byte loads: the elements in front of the first 16-byte boundary of the walked tensor (at
//           most three) and behind the last whole float4 (at most three) are taken one by one, so a base that is only
//           4-byte aligned is served at full width.  One group of four per thread and trip; a grid is one workgroup per
//           1,024 elements, at most MAX_WG of them; beyond MAX_WG * 1,024 elements a workgroup walks (grid-stride).  Any
//           other tensor of the call is accessed 16 bytes wide where it shares the walked tensor's alignment (`wide`)
//           and element by element where it does not.  walk_span is the one spelling of this: `walk` is it for the
//           grid over a tensor, ssg_chunked.hpp's walk_chunk for a workgroup over one chunk of a ragged set.
//   sums    each fp32 value is widened and ADDED IN FP64.  A thread adds its elements in index order, a wave folds by
//           the shuffle tree, a workgroup adds its four waves in order, pairwise: (w0 + w1) + (w2 + w3); one workgroup
//           folds the partials (thread i takes i, i + 256, ..., then an LDS tree).  No atomics, no tickets: the same
//           bits from call to call for the same n and pointer alignment.  A call of a single workgroup (n <= 1,024)
//           writes the result itself: one launch instead of two.
// pixel::block_sum (ssg_pixel.hpp) is a DIFFERENT sum: it adds the four waves left to right, ((w0 + w1) + w2) + w3, and
// the files built on it are pinned to those bits.
#pragma once
#include <math.h>

#include <type_traits>

#include "ssg_host.hpp"

namespace ssg {
namespace stream {

constexpr int NT = 256;        // threads per workgroup
constexpr int EPT = 4;         // elements per thread and trip: one float4
constexpr int MAX_WG = 1024;   // the grid cap (ssg_gan_grid_cap, ssg_spsr_grid_cap): four workgroups per CU

// the elements in front of x's first 16-byte boundary (x is 4-byte aligned)
__device__ __forceinline__ size_t head_of(const float *x, size_t n) {
  const size_t h = ((16 - ((size_t)x & 15)) & 15) / sizeof(float);
  return h < n ? h : n;
}

// does p share the walked tensor's alignment: is p + head on a 16-byte boundary
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

// THE walk, of which every other is a case: the span of n elements whose first `head` lie in front of a 16-byte boundary,
// for the threads first, first + stride, ...  A thread meets its elements in this order: one(e) for its element of the
// head, quad(e) for its groups e .. e + 3 (on a 16-byte boundary) in ascending order, one(e) for its element of the tail
// behind the last whole group.  I is the index type: size_t for a tensor, unsigned inside a chunk.
template <class I, class One, class Quad>
__device__ __forceinline__ void walk_span(I head, I n, I first, I stride, One one, Quad quad) {
  const I n4 = (n - head) / EPT;
  for (I e = first; e < head; e += stride) one(e);
  for (I q = first; q < n4; q += stride) quad(head + EPT * q);
  for (I e = head + EPT * n4 + first; e < n; e += stride) one(e);
}

// the flat walk of the whole grid over the n elements behind ptr (grid-stride)
template <class One, class Quad>
__device__ __forceinline__ void walk(const float *ptr, size_t n, One one, Quad quad) {
  walk_span<size_t>(head_of(ptr, n), n, (size_t)blockIdx.x * NT + threadIdx.x, (size_t)gridDim.x * NT, one, quad);
}

// l and l' of one difference d = p - q, every operation fp32 and rounded on its own (the files that use them are
// compiled with -ffp-contract=off): the pixel criteria of ssg_spsr.hip and ssg_mcrit.hip
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

// the workgroup's NV fp64 sums, dst[k] (every thread must call it; a caller that calls it again puts a barrier between)
template <int NV>
__device__ __forceinline__ void workgroup_fold(const double (&v)[NV], double *dst) {
  __shared__ double w[NV][NT / 64];
  double r[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) r[k] = v[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < NV; ++k) r[k] += __shfl_down(r[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) w[k][threadIdx.x >> 6] = r[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) dst[k] = (w[k][0] + w[k][1]) + (w[k][2] + w[k][3]);
  }
}

// NV fp64 partials per workgroup, part[NV * blockIdx.x + k] (every thread must call it)
template <int NV>
__device__ __forceinline__ void workgroup_partials(const double (&v)[NV], double *part) {
  workgroup_fold<NV>(v, part + NV * blockIdx.x);
}

// one workgroup folds nparts groups of NV partials into out[0 .. NV)
template <int NV, class Out>
__global__ __launch_bounds__(NT) void fold_kernel(const double *part, int nparts, Out *out) {
  __shared__ double s[NV][NT];
  double a[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) a[k] = 0.0;
  for (int i = threadIdx.x; i < nparts; i += NT) {
#pragma unroll
    for (int k = 0; k < NV; ++k) a[k] += part[NV * i + k];
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) s[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < NV; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) out[k] = (Out)s[k][0];
  }
}

// ---- host ----
// the pixel kinds, spelled out once: f(std::integral_constant<int, KIND>).  SSG_PIX_FRO is ssg_mcrit.hip's extra kind;
// without FRO no kernel of it is instantiated
template <bool FRO = false, class F>
inline void with_pixel_kind(int kind, F f) {
  if (kind == SSG_PIX_L1) f(std::integral_constant<int, SSG_PIX_L1>{});
  else if (kind == SSG_PIX_MSE) f(std::integral_constant<int, SSG_PIX_MSE>{});
  else if (FRO && kind == SSG_PIX_FRO) f(std::integral_constant<int, FRO ? SSG_PIX_FRO : SSG_PIX_CHARBONNIER>{});
  else f(std::integral_constant<int, SSG_PIX_CHARBONNIER>{});
}

inline unsigned grid_for(size_t n, int per_thread) {
  const size_t per = (size_t)NT * per_thread, want = (n + per - 1) / per;
  return (unsigned)(want < 1 ? 1 : (want > MAX_WG ? MAX_WG : want));
}

// where a sums kernel of `grid` workgroups writes: a single workgroup's partials are the result
inline double *partials_of(unsigned grid, void *workspace, double *out) { return grid == 1 ? out : (double *)workspace; }

// the partials' fold behind a sums kernel (a single workgroup has written `out` itself)
// (static: where a caller does not inline it, the library's dynamic symbols still stay as they were)
template <int NV, class Out>
static inline int finish_sums(unsigned grid, const double *part, Out *out, hipStream_t st) {
  if (grid > 1) hipLaunchKernelGGL((fold_kernel<NV, Out>), dim3(1), dim3(NT), 0, st, part, (int)grid, out);
  return (int)hipGetLastError();
}

}  // namespace stream
}  // namespace ssg
