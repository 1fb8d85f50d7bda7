// The kernels the degradation chain convolves with, made on the device (include/ssg_hip.h section (I)): the dataset's
// per-sample synthesis (basicsr/data/my_realesrgan_image_mask_dataset.py:88-141 through degradations.py:16-173,389-409
// -- numpy, np.linalg.inv, scipy.special.j1, np.pad on the CPU there) as one launch for a whole batch's records.
//
// One workgroup of 256 threads owns one pad_to x pad_to output (at most 21 x 21 = 441 elements: two per thread), so
// the normalising sum never leaves the workgroup: wave shuffles, four partials through LDS, the same order every time.
// Everything is fp64 -- Sigma's inverse, q, pow / exp / j1, the sum and the division; in fp32 the tails and the sum
// miss the reference's fp32 result by up to 2e4 ulps -- and the store is the only fp32 rounding.  The work is tiny
// (a batch of 16 samples is 48 workgroups): what a call costs is its one copy and its one launch.
// This file defines the entry point ssg_synth_kernels, at its end.
#include "../../include/ssg_hip.h"

#include "ssg_host.hpp"

namespace ssg {

constexpr int SYNTH_MAX_PAD = 21;     // the largest padded kernel (stock Real-ESRGAN's; filter2d's largest k)
constexpr int KSYN_NT = 256;          // threads per workgroup: >= SYNTH_MAX_PAD^2 / 2
constexpr int KSYN_MAX_GRID = 1024;   // workgroups per launch; workgroup b makes outputs b, b + grid, ...
static_assert(2 * KSYN_NT >= SYNTH_MAX_PAD * SYNTH_MAX_PAD, "two elements per thread cover the largest output");

// fixed-order sum over the workgroup, returned to every thread (every thread calls it; a barrier must separate two calls)
__device__ __forceinline__ double ksyn_block_sum(double v, double *sh) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
  for (int i = 1; i < KSYN_NT / 64; ++i) s += sh[i];
  return s;
}

// Sigma^-1 = (U diag(sig_x^2, sig_y^2) U^T)^-1 as {m00, m01, m11} (sigma_matrix2 + np.linalg.inv, closed form)
struct SymInv {
  double m00, m01, m11;
};
__device__ __forceinline__ SymInv sigma_inverse(double sig_x, double sig_y, double theta) {
  double s, c;
  sincos(theta, &s, &c);
  const double dx = sig_x * sig_x, dy = sig_y * sig_y;
  const double s00 = c * c * dx + s * s * dy, s01 = c * s * dx - s * c * dy, s11 = s * s * dx + c * c * dy;
  const double det = s00 * s11 - s01 * s01;
  return {s11 / det, -s01 / det, s00 / det};
}

// the un-normalised value of record r at column x, row y of its K x K grid (0 <= x, y < K)
__device__ __forceinline__ double kernel_value(const ssg_kernel_record &r, const SymInv &m, int x, int y) {
  const int K = r.size;
  if (r.kind == SSG_KERNEL_PULSE) return (x == K / 2 && y == K / 2) ? 1.0 : 0.0;
  if (r.kind == SSG_KERNEL_SINC) {   // degradations.py:400-404
    const double w = r.omega_c, c = (K - 1) / 2.0, dx = x - c, dy = y - c;
    if (x == (K - 1) / 2 && y == (K - 1) / 2) return w * w / (4.0 * M_PI);
    const double rad = sqrt(dy * dy + dx * dx);
    return w * j1(w * rad) / (2.0 * M_PI * rad);
  }
  const double gx = x - K / 2, gy = y - K / 2;   // mesh_grid: x along columns
  const double q = (gx * m.m00 + gy * m.m01) * gx + (gx * m.m01 + gy * m.m11) * gy;   // degradations.py:62
  if (r.kind == SSG_KERNEL_GAUSSIAN) return exp(-0.5 * q);
  const double p = pow(q, r.beta);
  return r.kind == SSG_KERNEL_GENERALIZED ? exp(-0.5 * p) : 1.0 / (p + 1.0);   // :138, :171
}

__global__ __launch_bounds__(KSYN_NT) void synth_kernels(const ssg_kernel_record *__restrict__ records, int n, int P,
                                                         float *__restrict__ out) {
  __shared__ double sh[KSYN_NT / 64];
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const ssg_kernel_record r = records[k];
    const int K = r.size, off = (P - K) / 2;
    const bool gauss = r.kind >= SSG_KERNEL_GAUSSIAN;
    const SymInv m = gauss ? sigma_inverse(r.sig_x, r.sig_y, r.theta) : SymInv{0.0, 0.0, 0.0};
    double v[2], part = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = threadIdx.x + j * KSYN_NT, row = i / P, x = i - row * P - off, y = row - off;
      // (the host has refused K > P; whatever a record says, nothing is written outside its own output)
      const bool inside = i < P * P && x >= 0 && x < K && y >= 0 && y < K;
      v[j] = inside ? kernel_value(r, m, x, y) : 0.0;
      part += v[j];
    }
    const double sum = ksyn_block_sum(part, sh);
    float *o = out + (size_t)k * P * P;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = threadIdx.x + j * KSYN_NT;
      if (i < P * P) o[i] = (float)(v[j] / sum);   // (a pulse's sum is 1)
    }
    __syncthreads();   // sh is written again on the next trip
  }
}

}  // namespace ssg

// ---- (I) the entry points: every refusal is decided here, before the launch ----
using namespace ssg;

extern "C" {

int ssg_synth_kernels(const ssg_kernel_record *records, int n, int pad_to, ssg_kernel_record *records_dev, float *out,
                      ssg_stream_t stream) {
  if (n < 0 || pad_to < 1 || pad_to > SYNTH_MAX_PAD || !(pad_to & 1)) return SSG_E_BADARG;
  if (n == 0) return 0;
  if (!records || !records_dev || !out) return SSG_E_BADARG;
  for (int i = 0; i < n; ++i) {
    const ssg_kernel_record &r = records[i];
    if (r.kind < SSG_KERNEL_PULSE || r.kind > SSG_KERNEL_PLATEAU) return SSG_E_BADARG;
    if (r.size < 1 || !(r.size & 1) || r.size > pad_to) return SSG_E_BADARG;
  }
  const int rc = (int)hipMemcpyAsync(records_dev, records, (size_t)n * sizeof(ssg_kernel_record), hipMemcpyHostToDevice,
                                     (hipStream_t)stream);
  if (rc) return rc;
  const unsigned grid = (unsigned)(n < KSYN_MAX_GRID ? n : KSYN_MAX_GRID);
  hipLaunchKernelGGL(synth_kernels, dim3(grid), dim3(KSYN_NT), 0, (hipStream_t)stream, records_dev, n, pad_to, out);
  return (int)hipGetLastError();
}

}  // extern "C"
