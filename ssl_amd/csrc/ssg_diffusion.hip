// What surrounds the Diffusion fork's U-Net, outside the network: the per-sample linear combinations of the schedule
// (Diffusion-Based-SR/ldm/models/diffusion/ddpm.py: q_sample, get_v, predict_start_from_noise,
// predict_start_from_z_and_v, q_posterior's mean), p_sample behind the network call, the training criterion of
// ddpmssl.py's p_losses, and the tile gather / weighted stitch of p_mean_variance_canvas (and, with unit weights, of
// scripts/util_image.py's ImageSpliterTh).
//
// Contract (this file is compiled with -ffp-contract=off; every fp32 operation is rounded on its own, in the
// reference's order, so on the same tables the elementwise results are torch's bits).  x is (B, n) fp32, sample b at
// x + b n: a sample's base needs only a float's alignment.  t is B int64 ON THE DEVICE and every table is T fp32 on the
// device; a coefficient is tab[t_b], gathered by the kernel.  A t_b outside [0, T) reads nothing: its coefficients are
// NaN, and so is everything of that sample.
//   combine    out = fl(fl(A[t_b] x) +- fl(B[t_b] y)), then the optional clamp (a NaN stays a NaN)
//   p_sample   x_recon = fl(fl(ra[t_b] x) - fl(rb[t_b] m)) (eps: sqrt_recip / sqrt_recipm1; v: sqrt_alphas_cumprod /
//              sqrt_one_minus) or m itself (x0); the optional clamp to [-1, 1]; mean = fl(fl(c1 x_recon) + fl(c2 x));
//              out = fl(mean + fl(fl(m_b sigma[t_b]) noise)), m_b = (t_b != 0); x_recon is written where asked for
//   loss_sums  one fp64 partial per chunk of sum_i l(target - pred), l = |d| or d d (stream::crit, fp32, widened)
//   loss_finish one workgroup: S_b = the sample's partials added in chunk order; in fp64, mean_b = S_b / n,
//              wbar = mean_b(p2[t_b]) (1 without the table), l_b = wbar mean_b / exp(logvar[t_b]) + logvar[t_b];
//              scalars = {mean_b(mean_b), mean_b(l_b), mean_b(lvlb[t_b] mean_b), lsw mean_b(l_b) + elbo mean_b(lvlb mean)};
//              coef_b = (lsw wbar / exp(logvar[t_b]) + elbo lvlb[t_b]) / B = dloss / dmean_b;
//              dlogvar[tau] = sum over the samples with t_b = tau, IN SAMPLE ORDER, of lsw (1 - wbar mean_b / exp(lv)) / B.
//              wbar, not p2[t_b]: the reference multiplies its (B,) loss_simple by a (B, 1, 1, 1) weight, so its loss is
//              the (B, 1, 1, B) array w_i mean_j / e_j + lv_j, and the mean of that weights every sample by the batch
//              mean of the P2 weights (ddpmssl.py:397-401).  Kept, as the fork's other quirks are.
//   loss_grad  grad[b, i] = (float)(g coef_b / n (double)(-l'(d))) - fl(rb[t_b] gx0[b, i]); the second term only
//              where gx0 is given: the gradient that arrives through x0 = predict_start_from_noise(x_noisy, t, pred)
//   gather     tiles[(k B + b), c, y, x] = src[b, c, oy_k + y, ox_k + x]
//   stitch     per output pixel, over the tiles that cover it IN TABLE ORDER: acc = (float)((double)acc + (double)pred
//              w64), cnt = (float)((double)cnt + w64), out = acc / cnt (one fp32 division): torch's in-place add of an
//              fp64 product into an fp32 tensor.  Without a weight table w64 = 1.
// Chunks of ssg_diff_chunk() elements of ONE sample, their schedule (at most ssg_diff_grid_cap() workgroups, further
// chunks grid-stride) and, for the elementwise kernels, their walk are ssg_chunked.hpp's: the walked tensor is the
// output, any other tensor is accessed 16 bytes wide where it shares its alignment.  The sums kernel does NOT use that
// walk: its threads take the groups of four by their index inside the chunk, whatever the alignment (scalar loads
// where the chunk is not on a 16-byte boundary), so that S_b does not depend on where the sample lies: sample b of a
// batch gives the bits of that sample alone.  One writer per output element, no atomics, no scratch; LDS holds the
// folds only.
// This file defines the ten entry points ssg_diff_*, at its end: they refuse bad arguments before any launch.
#include "ssg_chunked.hpp"

namespace ssg {
namespace diff {

using namespace chunked;

constexpr int CHUNK = 4096;        // elements per chunk: four float4 trips of a workgroup, as ssg_multi.hip's
constexpr int GRID_CAP = MAX_WG;   // the scaffold's: four workgroups per CU

SSG_TUNING tuning = {CHUNK, GRID_CAP};

typedef long long i64;

// tab[t], NaN for a t outside the table (nothing is read then)
__device__ __forceinline__ float coef_at(const float *tab, i64 t, int T) {
  return t >= 0 && t < (i64)T ? tab[t] : __builtin_nanf("");
}

__device__ __forceinline__ float clamped(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// where chunk c of the launch lies: its sample and its span inside the sample
struct Where { size_t b; Span sp; };

__device__ __forceinline__ Where where_of(size_t c, size_t cps, size_t n, unsigned chunk) {
  const size_t b = c / cps;
  return Where{b, span_of(n, c - b * cps, chunk)};
}

template <bool SUB, bool CLAMP>
__global__ __launch_bounds__(NT) void combine_kernel(const float *x, const float *y, const i64 *t, const float *A,
                                                     const float *Bt, int T, size_t total, size_t cps, size_t n,
                                                     unsigned chunk, float lo, float hi, float *out) {
  for (size_t c = blockIdx.x; c < total; c += gridDim.x) {
    const Where w = where_of(c, cps, n, chunk);
    const i64 tb = t[w.b];
    const float a = coef_at(A, tb, T), bb = coef_at(Bt, tb, T);
    const size_t base = w.b * n + w.sp.off;
    const float *px = x + base, *py = y + base;
    float *po = out + base;
    const size_t head = head_of(po, w.sp.len);
    const bool xv = wide(px, head), yv = wide(py, head);
    const auto f = [&](float u, float v) {
      const float p = a * u, q = bb * v;
      const float r = SUB ? p - q : p + q;
      return CLAMP ? clamped(r, lo, hi) : r;
    };
    walk_chunk(
        po, w.sp.len, [&](unsigned e) { po[e] = f(px[e], py[e]); },
        [&](unsigned e) {
          float u[4], v[4], r[4];
          load4(px + e, xv, u);
          load4(py + e, yv, v);
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = f(u[k], v[k]);
          store4(po + e, true, r);
        });
  }
}

template <int PARAM, bool CLIP, bool X0>
__global__ __launch_bounds__(NT) void p_sample_kernel(const float *x, const float *m, const float *noise, const i64 *t,
                                                      const float *ra, const float *rb, const float *c1,
                                                      const float *c2, const float *sigma, int T, size_t total,
                                                      size_t cps, size_t n, unsigned chunk, float *out, float *x0) {
  for (size_t c = blockIdx.x; c < total; c += gridDim.x) {
    const Where w = where_of(c, cps, n, chunk);
    const i64 tb = t[w.b];
    const float a = PARAM == SSG_DIFF_X0 ? 0.f : coef_at(ra, tb, T), bb = PARAM == SSG_DIFF_X0 ? 0.f : coef_at(rb, tb, T);
    const float k1 = coef_at(c1, tb, T), k2 = coef_at(c2, tb, T);
    const float s = (tb == 0 ? 0.f : 1.f) * coef_at(sigma, tb, T);
    const size_t base = w.b * n + w.sp.off;
    const float *px = x + base, *pm = m + base, *pz = noise + base;
    float *po = out + base, *p0 = X0 ? x0 + base : nullptr;
    const size_t head = head_of(po, w.sp.len);
    const bool xv = wide(px, head), mv = wide(pm, head), zv = wide(pz, head), v0 = X0 && wide(p0, head);
    const auto f = [&](float u, float v, float z, float &rec) {
      if (PARAM == SSG_DIFF_X0) {
        rec = v;
      } else {
        const float p = a * u, q = bb * v;
        rec = p - q;
      }
      if (CLIP) rec = clamped(rec, -1.f, 1.f);
      const float p1 = k1 * rec, p2 = k2 * u;
      const float mean = p1 + p2;
      const float sz = s * z;
      return mean + sz;
    };
    walk_chunk(
        po, w.sp.len,
        [&](unsigned e) {
          float rec;
          po[e] = f(px[e], pm[e], pz[e], rec);
          if (X0) p0[e] = rec;
        },
        [&](unsigned e) {
          float u[4], v[4], z[4], r[4], rec[4];
          load4(px + e, xv, u);
          load4(pm + e, mv, v);
          load4(pz + e, zv, z);
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = f(u[k], v[k], z[k], rec[k]);
          store4(po + e, true, r);
          if (X0) store4(p0 + e, v0, rec);
        });
  }
}

__device__ __forceinline__ bool on16(const float *p) { return (((size_t)p) & 15) == 0; }

// one fp64 partial per chunk; the threads take the chunk's groups of four BY INDEX (see the head of this file)
template <int KIND>
__global__ __launch_bounds__(NT) void loss_sums_kernel(const float *pred, const float *target, size_t total, size_t cps,
                                                       size_t n, unsigned chunk, double *part) {
  for (size_t c = blockIdx.x; c < total; c += gridDim.x) {
    const Where w = where_of(c, cps, n, chunk);
    const size_t base = w.b * n + w.sp.off;
    const float *p = pred + base, *g = target + base;
    const bool pv = on16(p), gv = on16(g);
    const unsigned n4 = w.sp.len / EPT;
    double L = 0.0;
    for (unsigned q = threadIdx.x; q < n4; q += NT) {
      float a[4], b[4];
      load4(p + EPT * q, pv, a);
      load4(g + EPT * q, gv, b);
#pragma unroll
      for (int k = 0; k < 4; ++k) L += (double)crit<KIND>(b[k] - a[k], 0.f);
    }
    const unsigned e = EPT * n4 + threadIdx.x;
    if (e < w.sp.len) L += (double)crit<KIND>(g[e] - p[e], 0.f);
    workgroup_fold<1>({L}, part + c);
    __syncthreads();   // (the fold's LDS words are written again in the next trip)
  }
}

// what the finishing kernel knows of sample b once S_b is there
struct Term { double mean, w, e, lv, vw; };

// wbar is the weight of EVERY sample: the batch mean of the P2 weights (see the head of this file), 1 without the table
__device__ __forceinline__ Term term_of(double S, double n, i64 tb, double wbar, const float *logvar, const float *lvlb,
                                        int T) {
  Term r;
  r.mean = S / n;
  r.w = tb >= 0 && tb < (i64)T ? wbar : (double)__builtin_nanf("");
  r.lv = (double)coef_at(logvar, tb, T);
  r.e = exp(r.lv);
  r.vw = (double)coef_at(lvlb, tb, T);
  return r;
}

__global__ __launch_bounds__(NT) void loss_finish_kernel(const double *part, size_t cps, const i64 *t, const float *p2,
                                                         const float *logvar, const float *lvlb, int T, int B, double n,
                                                         double lsw, double elbo, double *S, double *scalars,
                                                         double *coef, double *dlogvar) {
  double acc[3] = {0.0, 0.0, 0.0};
  double wbar = 1.0;
  if (p2) {   // every thread adds the B weights itself, in sample order: the same bits in all of them
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)coef_at(p2, t[b], T);
    wbar = s / (double)B;
  }
  for (int b = threadIdx.x; b < B; b += NT) {
    double s = 0.0;
    for (size_t k = 0; k < cps; ++k) s += part[(size_t)b * cps + k];
    S[b] = s;
    const Term r = term_of(s, n, t[b], wbar, logvar, lvlb, T);
    acc[0] += r.mean;
    acc[1] += r.w * r.mean / r.e + r.lv;
    acc[2] += r.vw * r.mean;
    coef[b] = (lsw * r.w / r.e + elbo * r.vw) / (double)B;
  }
  __threadfence_block();              // (S is read again below, by other threads of this workgroup)
  workgroup_fold<3>(acc, scalars);    // (a barrier inside)
  if (threadIdx.x == 0) {
    const double simple = scalars[0] / (double)B, gamma = scalars[1] / (double)B, vlb = scalars[2] / (double)B;
    scalars[0] = simple, scalars[1] = gamma, scalars[2] = vlb, scalars[3] = lsw * gamma + elbo * vlb;
  }
  if (dlogvar) {
    for (int tau = threadIdx.x; tau < T; tau += NT) {
      double d = 0.0;
      for (int b = 0; b < B; ++b) {
        if (t[b] != (i64)tau) continue;
        const Term r = term_of(S[b], n, (i64)tau, wbar, logvar, lvlb, T);
        d += lsw * (1.0 - r.w * r.mean / r.e) / (double)B;
      }
      dlogvar[tau] = d;
    }
  }
}

template <int KIND, bool X0>
__global__ __launch_bounds__(NT) void loss_grad_kernel(const float *pred, const float *target, const float *gx0,
                                                       const i64 *t, const float *rb, int T, const float *g,
                                                       const double *coef, size_t total, size_t cps, size_t n,
                                                       unsigned chunk, float *out) {
  const double g0 = (double)g[0];
  for (size_t c = blockIdx.x; c < total; c += gridDim.x) {
    const Where w = where_of(c, cps, n, chunk);
    const double cb = g0 * coef[w.b] / (double)n;
    const float r0 = X0 ? coef_at(rb, t[w.b], T) : 0.f;
    const size_t base = w.b * n + w.sp.off;
    const float *p = pred + base, *q = target + base, *z = X0 ? gx0 + base : nullptr;
    float *po = out + base;
    const size_t head = head_of(po, w.sp.len);
    const bool pv = wide(p, head), qv = wide(q, head), zv = X0 && wide(z, head);
    const auto f = [&](float a, float b, float u) {
      const float r = (float)(cb * (double)(-dcrit<KIND>(b - a, 0.f)));
      if (!X0) return r;
      const float back = r0 * u;
      return r - back;
    };
    walk_chunk(
        po, w.sp.len, [&](unsigned e) { po[e] = f(p[e], q[e], X0 ? z[e] : 0.f); },
        [&](unsigned e) {
          float a[4], b[4], u[4] = {0.f, 0.f, 0.f, 0.f}, r[4];
          load4(p + e, pv, a);
          load4(q + e, qv, b);
          if (X0) load4(z + e, zv, u);
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = f(a[k], b[k], u[k]);
          store4(po + e, true, r);
        });
  }
}

// ---- the canvas: tiles are records of three ints on the device, {oy, ox, src}; a record whose square leaves the
// canvas, or whose src leaves the tile tensor, is skipped by both kernels ----
struct Canvas {
  int B, C, h, w, ts, ntiles;
};

__device__ __forceinline__ bool tile_ok(const Canvas &cv, int oy, int ox) {
  return oy >= 0 && ox >= 0 && oy <= cv.h - cv.ts && ox <= cv.w - cv.ts;
}

__global__ __launch_bounds__(NT) void canvas_gather_kernel(const float *src, const int *tiles, Canvas cv, size_t total,
                                                           float *out) {
  const size_t ts = (size_t)cv.ts, per = (size_t)cv.C * ts * ts;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const size_t kb = i / per, r = i - kb * per;
    const size_t k = kb / (size_t)cv.B, b = kb - k * (size_t)cv.B;
    const size_t c = r / (ts * ts), yx = r - c * ts * ts, y = yx / ts, x = yx - y * ts;
    const int oy = tiles[3 * k], ox = tiles[3 * k + 1];
    if (!tile_ok(cv, oy, ox)) continue;
    out[i] = src[((b * cv.C + c) * cv.h + (size_t)oy + y) * cv.w + (size_t)ox + x];
  }
}

// preds: n_preds tiles of (C, ts, ts); tile k's contribution to sample b is preds[src_k + b bstep].  weights: fp64,
// element (b, c, y, x) of a tile at b wsb + c wsc + y ts + x (strides 0 for one plane shared); null: 1.
__global__ __launch_bounds__(NT) void canvas_stitch_kernel(const float *preds, const int *tiles, const double *weights,
                                                           Canvas cv, int n_preds, int bstep, size_t wsb, size_t wsc,
                                                           size_t total, float *out) {
  const size_t ts = (size_t)cv.ts, per = (size_t)cv.C * ts * ts;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const size_t x = i % (size_t)cv.w, y = (i / (size_t)cv.w) % (size_t)cv.h;
    const size_t bc = i / ((size_t)cv.w * cv.h), c = bc % (size_t)cv.C, b = bc / (size_t)cv.C;
    float acc = 0.f, cnt = 0.f;
    for (int k = 0; k < cv.ntiles; ++k) {
      const int oy = tiles[3 * k], ox = tiles[3 * k + 1], s0 = tiles[3 * k + 2];
      if (!tile_ok(cv, oy, ox)) continue;
      if ((int)y < oy || (int)y >= oy + cv.ts || (int)x < ox || (int)x >= ox + cv.ts) continue;
      const long long s = (long long)s0 + (long long)b * bstep;
      if (s0 < 0 || s >= (long long)n_preds) continue;
      const size_t ty = y - (size_t)oy, tx = x - (size_t)ox;
      const double wt = weights ? weights[b * wsb + c * wsc + ty * ts + tx] : 1.0;
      const double term = (double)preds[(size_t)s * per + (c * ts + ty) * ts + tx] * wt;
      acc = (float)((double)acc + term);
      cnt = (float)((double)cnt + wt);
    }
    out[i] = acc / cnt;
  }
}

static unsigned flat_grid(size_t total) {
  const size_t want = (total + NT - 1) / NT;
  return (unsigned)(want < 1 ? 1 : (want > (size_t)tuning.grid_cap ? (size_t)tuning.grid_cap : want));
}

// the chunks of a sample and of the call; false where the call's count does not fit an int
static bool chunks(size_t B, size_t n, size_t *per_sample, size_t *total) {
  const size_t cps = chunks_of(n, (size_t)tuning.chunk);
  if (B == 0 || cps == 0 || cps > (size_t)INT_MAX / B) return false;
  *per_sample = cps, *total = cps * B;
  return true;
}

// what every per-sample entry point checks of its shape: (B, n) with a chunk count that fits, a table of T entries
static int check_shape(size_t B, size_t n, int T, size_t *per_sample, size_t *total) {
  if (B < 1 || n < 1 || T < 1) return SSG_E_BADARG;
  return chunks(B, n, per_sample, total) ? 0 : SSG_E_TOOLARGE;
}

// the canvas (B, C, h, w), its tiles of (C, ts, ts) and the n_tiles of them in a tile tensor: each below 2^31 elements
static int check_canvas(int ntiles, int B, int C, int h, int w, int ts, long long n_tiles) {
  if (ntiles < 1 || B < 1 || C < 1 || h < 1 || w < 1 || ts < 1 || ts > h || ts > w || n_tiles < 1) return SSG_E_BADARG;
  const unsigned long long lim = 1ull << 31;
  if ((unsigned long long)B * C >= lim || (unsigned long long)B * C * h >= lim || (unsigned long long)B * C * h * w >= lim)
    return SSG_E_TOOLARGE;
  if ((unsigned long long)C * ts * ts >= lim || (unsigned long long)n_tiles * C * ts * ts >= lim) return SSG_E_TOOLARGE;
  return 0;
}

}  // namespace diff

}  // namespace ssg

// ---- (W) the entry points: every refusal is decided here, before the launch ----
using namespace ssg;
using namespace ssg::diff;

extern "C" {

int ssg_diff_chunk(void) { return tuning.chunk; }

int ssg_diff_grid_cap(void) { return tuning.grid_cap; }

size_t ssg_diff_workspace_bytes(size_t B, size_t n) {
  size_t cps = 0, total = 0;
  return chunks(B, n, &cps, &total) ? sizeof(double) * total : 0;
}

int ssg_diff_combine(const float *x, const float *y, const long long *t, const float *A, const float *Bt, int T,
                     size_t B, size_t n, int subtract, int clamp, float lo, float hi, float *out, ssg_stream_t stream) {
  size_t cps = 0, total = 0;
  if (!x || !y || !t || !A || !Bt || !out) return SSG_E_BADARG;
  if (clamp && !(lo <= hi)) return SSG_E_BADARG;   // (a NaN fails the comparison)
  if (const int rc = check_shape(B, n, T, &cps, &total)) return rc;
  if (unaligned(x, 4) || unaligned(y, 4) || unaligned(A, 4) || unaligned(Bt, 4) || unaligned(out, 4) || unaligned(t, 8))
    return SSG_E_ALIGN;
  const auto go = [&](auto sub, auto cl) {
    hipLaunchKernelGGL((combine_kernel<decltype(sub)::value, decltype(cl)::value>), dim3(grid_of(total, tuning)),
                       dim3(NT), 0, (hipStream_t)stream, x, y, t, A, Bt, T, total, cps, n, (unsigned)tuning.chunk, lo, hi,
                       out);
  };
  if (subtract && clamp) go(std::true_type{}, std::true_type{});
  else if (subtract) go(std::true_type{}, std::false_type{});
  else if (clamp) go(std::false_type{}, std::true_type{});
  else go(std::false_type{}, std::false_type{});
  return (int)hipGetLastError();
}

int ssg_diff_p_sample(const float *x, const float *model_out, const float *noise, const long long *t, const float *ra,
                      const float *rb, const float *c1, const float *c2, const float *sigma, int T, size_t B, size_t n,
                      int param, int clip, float *out, float *x0_out, ssg_stream_t stream) {
  size_t cps = 0, total = 0;
  if (!x || !model_out || !noise || !t || !c1 || !c2 || !sigma || !out) return SSG_E_BADARG;
  if (param < SSG_DIFF_EPS || param > SSG_DIFF_V || (param != SSG_DIFF_X0 && (!ra || !rb))) return SSG_E_BADARG;
  if (const int rc = check_shape(B, n, T, &cps, &total)) return rc;
  if (unaligned(x, 4) || unaligned(model_out, 4) || unaligned(noise, 4) || unaligned(ra, 4) || unaligned(rb, 4) ||
      unaligned(c1, 4) || unaligned(c2, 4) || unaligned(sigma, 4) || unaligned(out, 4) || unaligned(x0_out, 4) ||
      unaligned(t, 8))
    return SSG_E_ALIGN;
  const auto go = [&](auto pm, auto cl, auto x0) {
    hipLaunchKernelGGL((p_sample_kernel<decltype(pm)::value, decltype(cl)::value, decltype(x0)::value>),
                       dim3(grid_of(total, tuning)), dim3(NT), 0, (hipStream_t)stream, x, model_out, noise, t, ra, rb, c1,
                       c2, sigma, T, total, cps, n, (unsigned)tuning.chunk, out, x0_out);
  };
  const auto with_flags = [&](auto pm) {
    if (clip && x0_out) go(pm, std::true_type{}, std::true_type{});
    else if (clip) go(pm, std::true_type{}, std::false_type{});
    else if (x0_out) go(pm, std::false_type{}, std::true_type{});
    else go(pm, std::false_type{}, std::false_type{});
  };
  if (param == SSG_DIFF_EPS) with_flags(std::integral_constant<int, SSG_DIFF_EPS>{});
  else if (param == SSG_DIFF_X0) with_flags(std::integral_constant<int, SSG_DIFF_X0>{});
  else with_flags(std::integral_constant<int, SSG_DIFF_V>{});
  return (int)hipGetLastError();
}

int ssg_diff_loss_sums(const float *pred, const float *target, size_t B, size_t n, int kind, void *workspace,
                       size_t workspace_bytes, ssg_stream_t stream) {
  size_t cps = 0, total = 0;
  if (!pred || !target || !workspace || (kind != SSG_PIX_L1 && kind != SSG_PIX_MSE)) return SSG_E_BADARG;
  if (const int rc = check_shape(B, n, 1, &cps, &total)) return rc;
  if (workspace_bytes < sizeof(double) * total) return SSG_E_WORKSPACE;
  if (unaligned(pred, 4) || unaligned(target, 4) || unaligned(workspace, 8)) return SSG_E_ALIGN;
  const auto go = [&](auto kd) {
    hipLaunchKernelGGL(loss_sums_kernel<decltype(kd)::value>, dim3(grid_of(total, tuning)), dim3(NT), 0,
                       (hipStream_t)stream, pred, target, total, cps, n, (unsigned)tuning.chunk, (double *)workspace);
  };
  if (kind == SSG_PIX_L1) go(std::integral_constant<int, SSG_PIX_L1>{});
  else go(std::integral_constant<int, SSG_PIX_MSE>{});
  return (int)hipGetLastError();
}

int ssg_diff_loss_finish(const void *workspace, size_t workspace_bytes, const long long *t, const float *p2,
                         const float *logvar, const float *lvlb, int T, size_t B, size_t n, double l_simple_weight,
                         double original_elbo_weight, double *sums_out, double *scalars_out, double *coef_out,
                         double *dlogvar_out, ssg_stream_t stream) {
  size_t cps = 0, total = 0;
  if (!workspace || !t || !logvar || !lvlb || !sums_out || !scalars_out || !coef_out) return SSG_E_BADARG;
  if (l_simple_weight != l_simple_weight || original_elbo_weight != original_elbo_weight) return SSG_E_BADARG;
  if (const int rc = check_shape(B, n, T, &cps, &total)) return rc;
  if (B > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  if (workspace_bytes < sizeof(double) * total) return SSG_E_WORKSPACE;
  if (unaligned(workspace, 8) || unaligned(t, 8) || unaligned(p2, 4) || unaligned(logvar, 4) || unaligned(lvlb, 4) ||
      unaligned(sums_out, 8) || unaligned(scalars_out, 8) || unaligned(coef_out, 8) || unaligned(dlogvar_out, 8))
    return SSG_E_ALIGN;
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const double *)workspace, cps, t, p2,
                     logvar, lvlb, T, (int)B, (double)n, l_simple_weight, original_elbo_weight, sums_out, scalars_out,
                     coef_out, dlogvar_out);
  return (int)hipGetLastError();
}

int ssg_diff_loss_grad(const float *pred, const float *target, const float *grad_x0, const long long *t,
                       const float *rb, int T, const float *g, const double *coef, size_t B, size_t n, int kind,
                       float *grad_pred, ssg_stream_t stream) {
  size_t cps = 0, total = 0;
  if (!pred || !target || !g || !coef || !grad_pred || (kind != SSG_PIX_L1 && kind != SSG_PIX_MSE)) return SSG_E_BADARG;
  if (grad_x0 && (!t || !rb)) return SSG_E_BADARG;
  if (const int rc = check_shape(B, n, grad_x0 ? T : 1, &cps, &total)) return rc;
  if (unaligned(pred, 4) || unaligned(target, 4) || unaligned(grad_x0, 4) || unaligned(rb, 4) || unaligned(g, 4) ||
      unaligned(grad_pred, 4) || unaligned(t, 8) || unaligned(coef, 8))
    return SSG_E_ALIGN;
  const auto go = [&](auto kd, auto x0) {
    hipLaunchKernelGGL((loss_grad_kernel<decltype(kd)::value, decltype(x0)::value>), dim3(grid_of(total, tuning)),
                       dim3(NT), 0, (hipStream_t)stream, pred, target, grad_x0, t, rb, T, g, coef, total, cps, n,
                       (unsigned)tuning.chunk, grad_pred);
  };
  const auto with_x0 = [&](auto kd) {
    if (grad_x0) go(kd, std::true_type{});
    else go(kd, std::false_type{});
  };
  if (kind == SSG_PIX_L1) with_x0(std::integral_constant<int, SSG_PIX_L1>{});
  else with_x0(std::integral_constant<int, SSG_PIX_MSE>{});
  return (int)hipGetLastError();
}

int ssg_diff_canvas_gather(const float *src, const int *tiles, int ntiles, int B, int C, int h, int w, int ts,
                           float *out, ssg_stream_t stream) {
  if (!src || !tiles || !out) return SSG_E_BADARG;
  if (const int rc = check_canvas(ntiles, B, C, h, w, ts, (long long)ntiles * B)) return rc;
  if (unaligned(src, 4) || unaligned(tiles, 4) || unaligned(out, 4)) return SSG_E_ALIGN;
  const Canvas cv = {B, C, h, w, ts, ntiles};
  const size_t total = (size_t)ntiles * B * C * ts * ts;
  hipLaunchKernelGGL(canvas_gather_kernel, dim3(flat_grid(total)), dim3(NT), 0, (hipStream_t)stream, src, tiles, cv, total,
                     out);
  return (int)hipGetLastError();
}

int ssg_diff_canvas_stitch(const float *preds, int n_preds, int bstep, const int *tiles, int ntiles,
                           const double *weights, size_t wsb, size_t wsc, int B, int C, int h, int w, int ts,
                           float *out, ssg_stream_t stream) {
  if (!preds || !tiles || !out || (bstep != 0 && bstep != 1)) return SSG_E_BADARG;
  if (const int rc = check_canvas(ntiles, B, C, h, w, ts, n_preds)) return rc;
  if (unaligned(preds, 4) || unaligned(tiles, 4) || unaligned(out, 4) || unaligned(weights, 8)) return SSG_E_ALIGN;
  const Canvas cv = {B, C, h, w, ts, ntiles};
  const size_t total = (size_t)B * C * h * w;
  hipLaunchKernelGGL(canvas_stitch_kernel, dim3(flat_grid(total)), dim3(NT), 0, (hipStream_t)stream, preds, tiles, weights,
                     cv, n_preds, bstep, wsb, wsc, total, out);
  return (int)hipGetLastError();
}

}  // extern "C"
