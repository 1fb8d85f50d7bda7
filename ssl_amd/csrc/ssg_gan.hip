// The GAN criteria on the GPU, plain and relativistic: basicsr/losses/gan_loss.py:11-140 (GANLoss, MultiScaleGANLoss:
// vanilla, lsgan, wgan, wgan_softplus, hinge) and KAIR's train_BSGRAN/models/loss.py:135-172 (gan, ragan, lsgan, wgan,
// softplusgan), with the relativistic-average lines of the nine *ssl_model.py files (cri_gan(real - mean(fake), ...),
// realesrganssl_model.py:480-483, 509-515) and of model_ssl.py:346-353, 375-390.  x fp32, n >= 1 elements in any layout
// (the criteria are means over every element); nothing is copied to the host.
//
// Contract (this file is compiled with -ffp-contract=off).  Per element d = x - shift, ONE fp32 subtraction as the
// reference's own `real - torch.mean(fake)`; shift = 0 without a shift pointer (d = x exactly).  t = label, s = sign:
//   BCE       l = max(d, 0) - d t + log1p(exp(-|d|))          l' = sigmoid(d) - t
//   LS        l = (d - t)^2                                    l' = 2 (d - t)
//   LINEAR    l = s d                                          l' = s
//   SOFTPLUS  l = max(z, 0) + log1p(exp(-|z|)),  z = s d       l' = s sigmoid(z)
//   HINGE     l = max(z, 0),  z = 1 + s d                      l' = s where z > 0 or z is NaN (torch's ReLU backward:
//                                                                   zero where z <= 0, exactly 0 included), else 0
//   sigmoid(z) = 1 / (1 + e) for z >= 0, e / (1 + e) below, e = exp(-|z|): nothing overflows, d = +-100 gives 100 or 0.
//   Every operation is fp32 and rounded once; `max(v, 0)` is `v < 0 ? 0 : v`, so a NaN stays a NaN and reaches the sum.
//   sums    sums_out[0] = sum of l, sums_out[1] = sum of l': each fp32 value is widened and ADDED IN FP64.  A thread adds
//           its elements in index order, a wave folds by the shuffle tree, a workgroup adds its four waves in order, one
//           workgroup folds the partial pairs (thread i takes i, i + 256, ..., then an LDS tree).  No atomics, no
//           tickets: the same bits from call to call for the same n and pointer alignment.
//   grad    grad[i] = (float)(coef[0] * (double)l'(d_i) + coef[1]), coef two doubles on the device: coef[0] carries
//           upstream x weight / n, coef[1] the constant that flows back through a mean (0 without one).
// Two streaming kernels, 256 threads, 16-byte loads: the elements in front of the first 16-byte boundary of x (at most
// three) and behind the last whole float4 (at most three) are taken one by one, so a base that is only 4-byte aligned
// is served at full width; the gradient is stored 16 bytes wide where grad shares x's alignment, one by one otherwise.
// One workgroup per 1,024 elements, at most MAX_WG of them; beyond MAX_WG * 1,024 elements a workgroup walks.  A call
// of a single workgroup (n <= 1,024) writes sums_out itself: one launch instead of two.
#include <math.h>

#include "ssg_host.hpp"

namespace ssg {
namespace gan {

constexpr int NT = 256;        // threads per workgroup
constexpr int EPT = 4;         // elements per thread and trip: one float4
constexpr int MAX_WG = 1024;   // the grid cap (ssg_gan_grid_cap): four workgroups per CU

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// l and l' of one element, fp32
template <int KIND>
__device__ __forceinline__ void element(float d, float s, float t, float &l, float &dl) {
  if (KIND == SSG_GAN_BCE || KIND == SSG_GAN_SOFTPLUS) {
    const float z = KIND == SSG_GAN_BCE ? d : s * d;
    const float e = expf(-fabsf(z));
    const float r = 1.f / (1.f + e);
    const float sig = z < 0.f ? e * r : r;
    const float lp = log1pf(e);
    if (KIND == SSG_GAN_BCE) {
      l = (relu_keep_nan(z) - z * t) + lp;
      dl = sig - t;
    } else {
      l = relu_keep_nan(z) + lp;
      dl = s * sig;
    }
  } else if (KIND == SSG_GAN_LS) {
    const float q = d - t;
    l = q * q;
    dl = 2.f * q;
  } else if (KIND == SSG_GAN_LINEAR) {
    l = s * d;
    dl = s;
  } else {
    const float z = 1.f + s * d;
    l = relu_keep_nan(z);
    dl = z <= 0.f ? 0.f : s;
  }
}

// the elements in front of x's first 16-byte boundary (x is 4-byte aligned)
__device__ __forceinline__ size_t head_of(const float *x, size_t n) {
  const size_t h = ((16 - ((size_t)x & 15)) & 15) / sizeof(float);
  return h < n ? h : n;
}

template <int KIND>
__global__ __launch_bounds__(NT) void gan_sums_kernel(const float *x, size_t n, float s, float t, const float *shift,
                                                      double *part) {
  __shared__ double w0[NT / 64], w1[NT / 64];
  const float sh = shift ? shift[0] : 0.f;
  const size_t head = head_of(x, n), n4 = (n - head) / EPT;
  const size_t first = (size_t)blockIdx.x * NT + threadIdx.x, stride = (size_t)gridDim.x * NT;
  const float4 *x4 = (const float4 *)(x + head);
  double L = 0.0, D = 0.0;
  float l, dl;
#define SSG_GAN_ADD(v)                 \
  element<KIND>((v) - sh, s, t, l, dl); \
  L += (double)l;                      \
  D += (double)dl;
  for (size_t i = first; i < head; i += stride) { SSG_GAN_ADD(x[i]) }
  for (size_t i = first; i < n4; i += stride) {
    const float4 v = x4[i];
    SSG_GAN_ADD(v.x) SSG_GAN_ADD(v.y) SSG_GAN_ADD(v.z) SSG_GAN_ADD(v.w)
  }
  for (size_t i = head + EPT * n4 + first; i < n; i += stride) { SSG_GAN_ADD(x[i]) }
#undef SSG_GAN_ADD
  for (int o = 32; o > 0; o >>= 1) {
    L += __shfl_down(L, o, 64);
    D += __shfl_down(D, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    w0[threadIdx.x >> 6] = L;
    w1[threadIdx.x >> 6] = D;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = (w0[0] + w0[1]) + (w0[2] + w0[3]);
    part[2 * blockIdx.x + 1] = (w1[0] + w1[1]) + (w1[2] + w1[3]);
  }
}

__global__ __launch_bounds__(NT) void gan_fold_kernel(const double *part, int nparts, double *out) {
  __shared__ double s0[NT], s1[NT];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nparts; i += NT) {
    a += part[2 * i];
    b += part[2 * i + 1];
  }
  s0[threadIdx.x] = a;
  s1[threadIdx.x] = b;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s0[threadIdx.x] += s0[threadIdx.x + o];
      s1[threadIdx.x] += s1[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = s0[0];
    out[1] = s1[0];
  }
}

template <int KIND>
__global__ __launch_bounds__(NT) void gan_grad_kernel(const float *x, size_t n, float s, float t, const float *shift,
                                                      const double *coef, float *g) {
  const float sh = shift ? shift[0] : 0.f;
  const double c0 = coef[0], c1 = coef[1];
  const size_t head = head_of(x, n);
  const size_t first = (size_t)blockIdx.x * NT + threadIdx.x, stride = (size_t)gridDim.x * NT;
  float l, dl;
#define SSG_GAN_GRAD(v, out)            \
  element<KIND>((v) - sh, s, t, l, dl); \
  out = (float)(c0 * (double)dl + c1);
  if ((((size_t)(g + head)) & 15) == 0) {
    const size_t n4 = (n - head) / EPT;
    const float4 *x4 = (const float4 *)(x + head);
    float4 *g4 = (float4 *)(g + head);
    for (size_t i = first; i < head; i += stride) { SSG_GAN_GRAD(x[i], g[i]) }
    for (size_t i = first; i < n4; i += stride) {
      const float4 v = x4[i];
      float4 r;
      SSG_GAN_GRAD(v.x, r.x) SSG_GAN_GRAD(v.y, r.y) SSG_GAN_GRAD(v.z, r.z) SSG_GAN_GRAD(v.w, r.w)
      g4[i] = r;
    }
    for (size_t i = head + EPT * n4 + first; i < n; i += stride) { SSG_GAN_GRAD(x[i], g[i]) }
  } else {
    for (size_t i = first; i < n; i += stride) { SSG_GAN_GRAD(x[i], g[i]) }
  }
#undef SSG_GAN_GRAD
  (void)l;
}

inline unsigned grid_for(size_t n) {
  const size_t want = (n + (size_t)NT * EPT - 1) / ((size_t)NT * EPT);
  return (unsigned)(want < 1 ? 1 : (want > MAX_WG ? MAX_WG : want));
}

inline int check(const float *x, size_t n, int kind, float sign) {
  if (!x || n == 0 || kind < SSG_GAN_BCE || kind > SSG_GAN_HINGE || !(sign == 1.f || sign == -1.f)) return SSG_E_BADARG;
  if ((size_t)x % sizeof(float)) return SSG_E_ALIGN;   // (the head / float4 split assumes a float's own alignment)
  return 0;
}

template <int KIND>
inline void sums_kind(unsigned grid, const float *x, size_t n, float s, float t, const float *shift, double *part,
                      hipStream_t st) {
  hipLaunchKernelGGL(gan_sums_kernel<KIND>, dim3(grid), dim3(NT), 0, st, x, n, s, t, shift, part);
}

template <int KIND>
inline void grad_kind(unsigned grid, const float *x, size_t n, float s, float t, const float *shift, const double *coef,
                      float *g, hipStream_t st) {
  hipLaunchKernelGGL(gan_grad_kernel<KIND>, dim3(grid), dim3(NT), 0, st, x, n, s, t, shift, coef, g);
}

}  // namespace gan

int gan_grid_cap() { return gan::MAX_WG; }

size_t gan_workspace_bytes() { return sizeof(double) * 2 * gan::MAX_WG; }

int launch_gan_sums(const float *x, size_t n, int kind, float sign, float label, const float *shift, void *workspace,
                    double *sums_out, hipStream_t st) {
  using namespace gan;
  if (const int rc = check(x, n, kind, sign)) return rc;
  if (!workspace || !sums_out) return SSG_E_BADARG;
  if (((size_t)workspace | (size_t)sums_out) % sizeof(double)) return SSG_E_ALIGN;
  const unsigned grid = grid_for(n);
  double *part = grid == 1 ? sums_out : (double *)workspace;   // a single workgroup's pair is the result
  switch (kind) {
    case SSG_GAN_BCE: sums_kind<SSG_GAN_BCE>(grid, x, n, sign, label, shift, part, st); break;
    case SSG_GAN_LS: sums_kind<SSG_GAN_LS>(grid, x, n, sign, label, shift, part, st); break;
    case SSG_GAN_LINEAR: sums_kind<SSG_GAN_LINEAR>(grid, x, n, sign, label, shift, part, st); break;
    case SSG_GAN_SOFTPLUS: sums_kind<SSG_GAN_SOFTPLUS>(grid, x, n, sign, label, shift, part, st); break;
    default: sums_kind<SSG_GAN_HINGE>(grid, x, n, sign, label, shift, part, st); break;
  }
  if (grid > 1) hipLaunchKernelGGL(gan_fold_kernel, dim3(1), dim3(NT), 0, st, (const double *)part, (int)grid, sums_out);
  return (int)hipGetLastError();
}

int launch_gan_grad(const float *x, size_t n, int kind, float sign, float label, const float *shift, const double *coef,
                    float *grad, hipStream_t st) {
  using namespace gan;
  if (const int rc = check(x, n, kind, sign)) return rc;
  if (!coef || !grad) return SSG_E_BADARG;
  if ((size_t)coef % sizeof(double) || (size_t)grad % sizeof(float)) return SSG_E_ALIGN;
  const unsigned grid = grid_for(n);
  switch (kind) {
    case SSG_GAN_BCE: grad_kind<SSG_GAN_BCE>(grid, x, n, sign, label, shift, coef, grad, st); break;
    case SSG_GAN_LS: grad_kind<SSG_GAN_LS>(grid, x, n, sign, label, shift, coef, grad, st); break;
    case SSG_GAN_LINEAR: grad_kind<SSG_GAN_LINEAR>(grid, x, n, sign, label, shift, coef, grad, st); break;
    case SSG_GAN_SOFTPLUS: grad_kind<SSG_GAN_SOFTPLUS>(grid, x, n, sign, label, shift, coef, grad, st); break;
    default: grad_kind<SSG_GAN_HINGE>(grid, x, n, sign, label, shift, coef, grad, st); break;
  }
  return (int)hipGetLastError();
}

}  // namespace ssg
