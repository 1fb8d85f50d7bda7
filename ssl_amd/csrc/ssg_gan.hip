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
//   sums    sums_out[0] = sum of l, sums_out[1] = sum of l', each fp32 value widened and added in fp64 in the fixed
//           order of ssg_stream.hpp: the same bits from call to call for the same n and pointer alignment.
//   grad    grad[i] = (float)(coef[0] * (double)l'(d_i) + coef[1]), coef two doubles on the device: coef[0] carries
//           upstream x weight / n, coef[1] the constant that flows back through a mean (0 without one).
// Two streaming kernels on ssg_stream.hpp's walk of x and its launch geometry; the gradient is stored 16 bytes wide where
// grad shares x's alignment; where it does not, x and grad are both taken one by one.  A call of a single workgroup
// (n <= 1,024) writes sums_out itself.
// This file defines the entry points ssg_gan_workspace_bytes, ssg_gan_grid_cap, ssg_gan_sums and ssg_gan_grad, at its end:
// they refuse bad arguments before any launch.
#include <math.h>

#include <type_traits>

#include "ssg_stream.hpp"

namespace ssg {
namespace gan {

using namespace stream;

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

template <int KIND>
__global__ __launch_bounds__(NT) void gan_sums_kernel(const float *x, size_t n, float s, float t, const float *shift,
                                                      double *part) {
  const float sh = shift ? shift[0] : 0.f;
  double L = 0.0, D = 0.0;
  const auto one = [&](size_t e) {
    float l, dl;
    element<KIND>(x[e] - sh, s, t, l, dl);
    L += (double)l;
    D += (double)dl;
  };
  const auto quad = [&](size_t e) {
    float v[4], l, dl;
    load4(x + e, true, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      element<KIND>(v[k] - sh, s, t, l, dl);
      L += (double)l;
      D += (double)dl;
    }
  };
  walk(x, n, one, quad);
  workgroup_partials<2>({L, D}, part);
}

template <int KIND>
__global__ __launch_bounds__(NT) void gan_grad_kernel(const float *x, size_t n, float s, float t, const float *shift,
                                                      const double *coef, float *g) {
  const float sh = shift ? shift[0] : 0.f;
  const double c0 = coef[0], c1 = coef[1];
  const auto grad_of = [&](float v) {
    float l, dl;
    element<KIND>(v - sh, s, t, l, dl);
    return (float)(c0 * (double)dl + c1);
  };
  const auto one = [&](size_t e) { g[e] = grad_of(x[e]); };
  if (wide(g, head_of(x, n))) {
    walk(x, n, one, [&](size_t e) {
      float v[4], r[4];
      load4(x + e, true, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = grad_of(v[k]);
      store4(g + e, true, r);
    });
  } else {
    const size_t stride = (size_t)gridDim.x * NT;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) one(e);
  }
}

// the family's kinds, spelled out once: f(std::integral_constant<int, KIND>)
template <class F>
inline void with_kind(int kind, F f) {
  switch (kind) {
    case SSG_GAN_BCE: f(std::integral_constant<int, SSG_GAN_BCE>{}); break;
    case SSG_GAN_LS: f(std::integral_constant<int, SSG_GAN_LS>{}); break;
    case SSG_GAN_LINEAR: f(std::integral_constant<int, SSG_GAN_LINEAR>{}); break;
    case SSG_GAN_SOFTPLUS: f(std::integral_constant<int, SSG_GAN_SOFTPLUS>{}); break;
    default: f(std::integral_constant<int, SSG_GAN_HINGE>{}); break;
  }
}

// what both entry points check of the logits
static int gan_check(const float *x, size_t n, int kind, float sign) {
  if (!x || n == 0 || kind < SSG_GAN_BCE || kind > SSG_GAN_HINGE || !(sign == 1.f || sign == -1.f)) return SSG_E_BADARG;
  return unaligned(x, 4) ? SSG_E_ALIGN : 0;   // (the head / float4 split assumes a float's own alignment)
}

}  // namespace gan

}  // namespace ssg

// ---- (Q) the entry points: every refusal is decided here, before the launch ----
using namespace ssg;

extern "C" {

size_t ssg_gan_workspace_bytes(void) { return sizeof(double) * 2 * gan::MAX_WG; }

int ssg_gan_grid_cap(void) { return gan::MAX_WG; }

int ssg_gan_sums(const float *x, size_t n, int kind, float sign, float label, const float *shift, void *workspace,
                 double *sums_out, ssg_stream_t stream) {
  using namespace gan;
  if (const int rc = gan_check(x, n, kind, sign)) return rc;
  if (!workspace || !sums_out) return SSG_E_BADARG;
  if (unaligned(workspace, 8) || unaligned(sums_out, 8)) return SSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(n, EPT);
  double *part = partials_of(grid, workspace, sums_out);
  with_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(gan_sums_kernel<decltype(k)::value>, dim3(grid), dim3(NT), 0, st, x, n, sign, label, shift, part);
  });
  return finish_sums<2>(grid, part, sums_out, st);
}

int ssg_gan_grad(const float *x, size_t n, int kind, float sign, float label, const float *shift, const double *coef,
                 float *grad, ssg_stream_t stream) {
  using namespace gan;
  if (const int rc = gan_check(x, n, kind, sign)) return rc;
  if (!coef || !grad) return SSG_E_BADARG;
  if (unaligned(coef, 8) || unaligned(grad, 4)) return SSG_E_ALIGN;
  with_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(gan_grad_kernel<decltype(k)::value>, dim3(grid_for(n, EPT)), dim3(NT), 0, (hipStream_t)stream, x, n,
                       sign, label, shift, coef, grad);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
