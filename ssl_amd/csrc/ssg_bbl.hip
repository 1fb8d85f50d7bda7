// BebyGAN's best-buddy loss and flat mask on the GPU: GAN-Based-SR/basicsr/models/bebyganssl_model.py:471-565
// (BBL.forward), its caller's L1Loss(p1, sel_p2) at :723-724 and get_flat_mask at :93-104.
//
// Contract (x = output, g = GT, each (B,C,H,W) fp32; k = ksize, s = stride >= k, pad = 0, d = C k^2 <= 31):
//   u(t)   = F.unfold(t, k, stride = s).permute(0, 2, 1)                      (B, n(t), d), element c k^2 + dy k + dx
//   p1 = u(x), p2 = u(g), N = n(x);  g2, g4 = bicubic (A = -0.75, align_corners = False, no antialias) 1/2 and 1/4 of g:
//            output side floor(side / 2 | / 4), every sample at fraction 0.5 of its source cell, so the four taps per
//            axis are -0.09375, 0.59375, 0.59375, -0.09375 at source 2y-1 .. 2y+2 (1/2) or 4y .. 4y+3 (1/4), clamped
//   cand   = cat[p2, u(g2), u(g4)]                                              (B, M, d)
//   score  = alpha |p1_i - cand_j|^2 + beta |p2_i - cand_j|^2, ind_i = argmin_j, the LOWEST j among equal fp32 scores
//   loss   = loss_weight mean |p1 - cand[ind]| (or the sum);  d loss / d x = loss_weight / (B N d) sgn(p1 - cand[ind])
//            at the pixel of each patch element (s >= k: every pixel lies in at most one patch), 0 elsewhere; sgn(0) = 0
// Only the j-dependent part of the score decides the argmin:
//   score'_ij = (alpha + beta) |cand_j|^2 - 2 (alpha p1_i + beta p2_i) . cand_j
// which is ONE matrix product with K = d + 1: rows [-2 q_i, 1], columns [cand_j, (alpha + beta) |cand_j|^2].
//
// Four launches per loss call, no atomics, every sum in a fixed order (bit-reproducible), no score matrix anywhere:
//   bbl_pack    one workgroup per 32 rows / candidates: the K-padded operands in 32 x 32 blocks stored k-major
//               ([block][kk][32 rows or candidates]), so that one step of the 32x32x2 MFMA reads 64 consecutive floats;
//               the two pyramid levels are formed here from the fixed 4 x 4 taps.  Padding candidates carry +inf in
//               their norm slot and never win.  Writes p1 when the caller wants it.
//   bbl_search  one wave per 32 rows: the rows' operand stays in registers (one VGPR per k step), candidate blocks of 32
//               stream through v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fmaf chain, so the scores are plain fp32);
//               each lane keeps (min, index) of its 16 accumulator rows over the candidates of its column, ascending
//               with a strict <, and the 32 lanes of a row are folded once at the end with lowest-index ties.  Small
//               batches split the candidate range over up to 8 workgroups (fixed by the shape alone).
//   bbl_loss    one thread per pixel: folds the splits' partial minima in ascending candidate order, gathers
//               cand[ind] from the packed operand, writes ind / sel_p2 / the gradient (its zeros included) and one
//               fp64 partial of sum |p1 - sel| per workgroup.
//   bbl_fold    one workgroup: the loss from the partials, in index order.
// get_flat_mask: one launch, a 32 x 16 tile per workgroup, luminance formed on load into an LDS tile with a reflect halo,
// two-pass unbiased variance, the threshold at the store (the layout of ssg_ldl.hip's ldl_map).
// Compiled with -ffp-contract=off (csrc/Makefile): the luminance (0.2989 r + 0.587 g) + 0.114 b is rounded product by
// product like the reference's torch expression.
#include <math.h>

#include "ssg_pixel.hpp"

namespace ssg {
namespace bbl {

using namespace pixel;             // NT, sgnf, block_sum, the flat mask's 32 x 16 tile and its reflect halo

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BLK = 32;            // rows / candidates per operand block (the MFMA tile side)
constexpr int KP = 32;             // padded K of a stored block: BLK * KP floats = 4 KiB
constexpr int DMAX = KP - 1;       // d + 1 <= KP
constexpr int MAX_SPLIT = 8;       // candidate ranges per row block at most
constexpr int WAVES_WANTED = 2048; // 2 waves for each of the 1,024 SIMDs

struct Args {
  const float *x, *g;   // (B,C,H,W)
  float *QT;            // (B, nrb, KP, BLK): rows [-2 (alpha p1 + beta p2), 1, 0 ...], k-major
  float *CT;            // (B, ncb, KP, BLK): columns [cand, (alpha + beta) |cand|^2, 0 ...], k-major
  float *pmin;          // (B, nsplit, nrb * BLK) partial minima
  int *pidx;            //                        and their candidate indices
  double *part;         // (B * nb3) sum |p1 - sel| of bbl_loss's workgroups
  int *ind;             // (B, N), nullable
  float *p1, *sel;      // (B, N, d), nullable
  float *grad;          // (B,C,H,W), nullable
  float *loss;          // 1 float, nullable
  float alpha, beta, scale;
  double loss_scale;
  int B, C, H, W, k, s, d;
  int nw, N;            // level 0 patch grid (nw patches per row)
  int H2, W2, nw2, N2;  // level 1/2
  int H4, W4, nw4, N4;  // level 1/4
  int M, nrb, ncb, nsplit, cbs, nb3;
};

// one sample of the bicubic 1/2 (sh = 1) or 1/4 (sh = 2) level of an H x W plane
__device__ __forceinline__ float level_sample(const float *p, int H, int W, int sh, int y, int x) {
  const float w[4] = {-0.09375f, 0.59375f, 0.59375f, -0.09375f};
  const int y0 = (y << sh) - (sh == 1), x0 = (x << sh) - (sh == 1);
  float v = 0.f;
  for (int r = 0; r < 4; ++r) {
    const float *row = p + (size_t)min(max(y0 + r, 0), H - 1) * W;
    float h = 0.f;
    for (int c = 0; c < 4; ++c) h += w[c] * row[min(max(x0 + c, 0), W - 1)];
    v += w[r] * h;
  }
  return v;
}

// ---------------------------------------------------------------------------------------------------------- pack ---
// One workgroup per operand block: thread t serves row / candidate t & 31 of the block and the k slots g, g + 8, g + 16,
// g + 24 with g = t >> 5, so every one of the block's 32 x 32 words is written once (32 consecutive floats per slot) and
// a thread forms at most four samples.  A candidate's |cand|^2 is the sum of the eight threads' partial sums (each over
// its slots in ascending order), folded in the order g = 0 .. 7.
__global__ __launch_bounds__(NT) void bbl_pack(Args a) {
  __shared__ float sq[NT / BLK][BLK];
  const int b = blockIdx.y, lane = threadIdx.x & (BLK - 1), g = threadIdx.x / BLK;
  const int HW = a.H * a.W, kk2 = a.k * a.k;
  const float *xb = a.x + (size_t)b * a.C * HW, *gb = a.g + (size_t)b * a.C * HW;
  if ((int)blockIdx.x < a.nrb) {
    const int i = blockIdx.x * BLK + lane;
    float *dst = a.QT + ((size_t)b * a.nrb + blockIdx.x) * (KP * BLK) + lane;
    const bool live = i < a.N;
    const int y0 = live ? (i / a.nw) * a.s : 0, x0 = live ? (i % a.nw) * a.s : 0;
    float *p1 = a.p1 && live ? a.p1 + ((size_t)b * a.N + i) * a.d : nullptr;
    for (int kk = g; kk < KP; kk += NT / BLK) {
      float v = live && kk == a.d ? 1.f : 0.f;
      if (live && kk < a.d) {
        const int c = kk / kk2, r = kk - c * kk2, dy = r / a.k, dx = r - dy * a.k;
        const size_t at = (size_t)c * HW + (size_t)(y0 + dy) * a.W + (x0 + dx);
        const float xv = xb[at];
        v = -2.f * (a.alpha * xv + a.beta * gb[at]);
        if (p1) p1[kk] = xv;
      }
      dst[kk * BLK] = v;
    }
    return;   // (the whole workgroup: no barrier on this side)
  }
  const int cb = blockIdx.x - a.nrb, j = cb * BLK + lane;
  float *dst = a.CT + ((size_t)b * a.ncb + cb) * (KP * BLK) + lane;
  const bool live = j < a.M;
  int sh = 0, jl = j, nw = a.nw;
  if (j >= a.N + a.N2) {
    sh = 2, jl = j - a.N - a.N2, nw = a.nw4;
  } else if (j >= a.N) {
    sh = 1, jl = j - a.N, nw = a.nw2;
  }
  const int y0 = live ? (jl / nw) * a.s : 0, x0 = live ? (jl % nw) * a.s : 0;
  float nrm = 0.f;
  for (int kk = g; kk < KP; kk += NT / BLK) {
    if (kk == a.d) continue;   // the norm slot, written below
    float v = 0.f;
    if (live && kk < a.d) {
      const int c = kk / kk2, r = kk - c * kk2, dy = r / a.k, dx = r - dy * a.k;
      const float *plane = gb + (size_t)c * HW;
      v = sh == 0 ? plane[(size_t)(y0 + dy) * a.W + (x0 + dx)] : level_sample(plane, a.H, a.W, sh, y0 + dy, x0 + dx);
      nrm += v * v;
    }
    dst[kk * BLK] = v;
  }
  sq[g][lane] = nrm;
  __syncthreads();
  if (g == a.d % (NT / BLK)) {
    float n = sq[0][lane];
    for (int t = 1; t < NT / BLK; ++t) n += sq[t][lane];
    // a padding candidate scores +inf, which the strict < of the search never takes
    dst[a.d * BLK] = live ? (a.alpha + a.beta) * n : INFINITY;
  }
}

// -------------------------------------------------------------------------------------------------------- search ---
// KS steps of the x2 MFMA cover K = 2 KS >= d + 1 (14 for d <= 27: C = 3, k = 3; 16 for the rest of the domain).
// MFMA 32x32x2 f32 operand maps: lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31]; accumulator
// register r of lane l is C[row (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col l & 31].  With the k-major blocks both operands
// of step t are the 64 consecutive floats at 64 t.
template <int KS>
__global__ __launch_bounds__(NT) void bbl_search(Args a) {
  const int lane = threadIdx.x & 63;
  const int rb = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const int split = blockIdx.y, b = blockIdx.z;
  if (rb >= a.nrb) return;   // wave-uniform; the kernel has no barrier
  const float *qt = a.QT + ((size_t)b * a.nrb + rb) * (KP * BLK) + lane;
  float av[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) av[t] = qt[t * 64];
  const int cb0 = split * a.cbs, cb1 = min(cb0 + a.cbs, a.ncb);
  float best[16];
  int bidx[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    best[r] = INFINITY;
    bidx[r] = 0;
  }
  const float *ct = a.CT + ((size_t)b * a.ncb + cb0) * (KP * BLK) + lane;
  float bv[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) bv[t] = ct[t * 64];
  for (int cb = cb0; cb < cb1; ++cb) {
    // the next block's operand is requested before this block's products are formed (the last iteration re-reads
    // its own block: in bounds, unused)
    const float *nx = ct + (cb + 1 < cb1 ? KP * BLK : 0);
    float nv[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t) nv[t] = nx[t * 64];
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KS; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc, 0, 0, 0);
    const int j = cb * BLK + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool lt = acc[r] < best[r];
      best[r] = lt ? acc[r] : best[r];
      bidx[r] = lt ? j : bidx[r];
    }
#pragma unroll
    for (int t = 0; t < KS; ++t) bv[t] = nv[t];
    ct = nx;
  }
  // the 32 lanes of a half hold one row's candidates by column: smallest score, then smallest index
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best[r], off);
      const int oi = __shfl_xor(bidx[r], off);
      const bool take = ov < best[r] || (ov == best[r] && oi < bidx[r]);
      best[r] = take ? ov : best[r];
      bidx[r] = take ? oi : bidx[r];
    }
  }
  if ((lane & 31) == 0) {
    const size_t base = ((size_t)b * a.nsplit + split) * ((size_t)a.nrb * BLK) + (size_t)rb * BLK;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      a.pmin[base + row] = best[r];
      a.pidx[base + row] = bidx[r];
    }
  }
}

// ------------------------------------------------------------------------------------- gather, loss and gradient ---
__global__ __launch_bounds__(NT) void bbl_loss(Args a) {
  __shared__ double sh[NT / 64];
  const int b = blockIdx.y, HW = a.H * a.W;
  const int p = blockIdx.x * NT + threadIdx.x;
  double lsum = 0.0;
  if (p < HW) {
    const int y = p / a.W, x = p - y * a.W;
    const int py = y / a.s, dy = y - py * a.s, px = x / a.s, dx = x - px * a.s;
    const size_t at = (size_t)b * a.C * HW + p;
    if (dy < a.k && dx < a.k && px < a.nw && py * a.nw + px < a.N) {
      const int i = py * a.nw + px;
      const size_t rows = (size_t)a.nrb * BLK;
      // the splits cover ascending candidate ranges: a strict < keeps the lowest index among equal scores
      float bm = a.pmin[(size_t)b * a.nsplit * rows + i];
      int j = a.pidx[(size_t)b * a.nsplit * rows + i];
      for (int sp = 1; sp < a.nsplit; ++sp) {
        const float v = a.pmin[((size_t)b * a.nsplit + sp) * rows + i];
        if (v < bm) {
          bm = v;
          j = a.pidx[((size_t)b * a.nsplit + sp) * rows + i];
        }
      }
      if (a.ind && dy == 0 && dx == 0) a.ind[(size_t)b * a.N + i] = j;
      const float *cand = a.CT + ((size_t)b * a.ncb + (j / BLK)) * (KP * BLK) + (j % BLK);
      for (int c = 0; c < a.C; ++c) {
        const int kk = c * a.k * a.k + dy * a.k + dx;
        const float sv = cand[kk * BLK];
        const float df = a.x[at + (size_t)c * HW] - sv;
        lsum += (double)fabsf(df);
        if (a.sel) a.sel[((size_t)b * a.N + i) * a.d + kk] = sv;
        if (a.grad) a.grad[at + (size_t)c * HW] = a.scale * sgnf(df);
      }
    } else if (a.grad) {
      for (int c = 0; c < a.C; ++c) a.grad[at + (size_t)c * HW] = 0.f;
    }
  }
  if (a.loss) {
    const double s = block_sum(lsum, sh);
    if (threadIdx.x == 0) a.part[(size_t)b * a.nb3 + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(NT) void bbl_fold(Args a) {
  __shared__ double sh[NT / 64];
  double l = 0.0;
  for (int i = threadIdx.x; i < a.B * a.nb3; i += NT) l += a.part[i];
  l = block_sum(l, sh);
  if (threadIdx.x == 0) a.loss[0] = (float)(a.loss_scale * l);
}

// ----------------------------------------------------------------------------------------------------- flat mask ---
template <int KT>
__global__ __launch_bounds__(NT) void flat_mask(const float *img, float *mask, int H, int W, int k, float thresh,
                                                int tiles_x) {
  __shared__ float sl[LH][LW];
  const int K = KT ? KT : k, R = K / 2;
  const int b = blockIdx.y, HW = H * W;
  const int tx0 = (blockIdx.x % tiles_x) * TW, ty0 = (blockIdx.x / tiles_x) * TH;
  const float *r = img + (size_t)b * 3 * HW, *g = r + HW, *bl = g + HW;
  load_halo_tile(sl, ty0, tx0, R, H, W, [&](int at) { return (0.2989f * r[at] + 0.587f * g[at]) + 0.114f * bl[at]; });
  __syncthreads();
  const float inv_n = 1.f / (float)(K * K), inv_n1 = 1.f / (float)(K * K - 1);
  const int lx = threadIdx.x & (TW - 1);
  for (int h = 0; h < 2; ++h) {
    const int ly = (threadIdx.x / TW) + h * (TH / 2);
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    float s = 0.f;
    for (int dy = 0; dy < K; ++dy)
      for (int dx = 0; dx < K; ++dx) s += sl[ly + dy][lx + dx];
    const float mu = s * inv_n;
    float q = 0.f;
    for (int dy = 0; dy < K; ++dy)
      for (int dx = 0; dx < K; ++dx) {
        const float d = sl[ly + dy][lx + dx] - mu;
        q += d * d;
      }
    mask[(size_t)b * HW + (size_t)y * W + x] = sqrtf(q * inv_n1) < thresh ? 1.f : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------- host ---
struct Layout {
  size_t QT, CT, pmin, pidx, part, total;
};

// geometry of a call: everything in Args but the pointers and weights
inline void geometry(Args &a, int B, int C, int H, int W, int k, int s) {
  a.B = B, a.C = C, a.H = H, a.W = W, a.k = k, a.s = s, a.d = C * k * k;
  a.nw = (W - k) / s + 1;
  a.N = ((H - k) / s + 1) * a.nw;
  a.H2 = H / 2, a.W2 = W / 2, a.H4 = H / 4, a.W4 = W / 4;
  a.nw2 = (a.W2 - k) / s + 1;
  a.N2 = ((a.H2 - k) / s + 1) * a.nw2;
  a.nw4 = (a.W4 - k) / s + 1;
  a.N4 = ((a.H4 - k) / s + 1) * a.nw4;
  a.M = a.N + a.N2 + a.N4;
  a.nrb = (a.N + BLK - 1) / BLK;
  a.ncb = (a.M + BLK - 1) / BLK;
  // candidate ranges per row block: enough waves to fill the chip, decided by the shape alone
  const long waves = (long)B * a.nrb;
  int ns = (int)((WAVES_WANTED + waves - 1) / waves);
  ns = ns < 1 ? 1 : ns > MAX_SPLIT ? MAX_SPLIT : ns;
  ns = ns > a.ncb ? a.ncb : ns;
  a.cbs = (a.ncb + ns - 1) / ns;
  a.nsplit = (a.ncb + a.cbs - 1) / a.cbs;
  a.nb3 = (H * W + NT - 1) / NT;
}

inline Layout layout(const Args &a) {
  Layout L;
  const size_t blk = sizeof(float) * KP * BLK;
  Carver c;
  L.QT = c.take(blk * a.B * a.nrb);
  L.CT = c.take(blk * a.B * a.ncb);
  L.pmin = c.take(sizeof(float) * (size_t)a.B * a.nsplit * a.nrb * BLK);
  L.pidx = c.take(sizeof(int) * (size_t)a.B * a.nsplit * a.nrb * BLK);
  L.part = c.take(sizeof(double) * (size_t)a.B * a.nb3);
  L.total = c.end;
  return L;
}

// argument checks shared by the entry points, in the order the header documents
inline int check_shape(int B, int C, int H, int W, int k, int s) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0 || s < k) return SSG_E_BADARG;
  if ((long)C * k * k > DMAX || B > 65535 || (double)B * C * H * W >= 2147483648.0) return SSG_E_TOOLARGE;
  if (H / 4 < k || W / 4 < k) return SSG_E_IMAGESMALL;
  return 0;
}

inline int prepare(Args &a, const float *x, const float *g, int B, int C, int H, int W, int k, int s, float alpha,
                   float beta, void *ws, size_t ws_bytes) {
  if (!(alpha >= 0.f) || !(beta >= 0.f) || !(alpha + beta > 0.f)) return SSG_E_BADARG;
  const int rc = check_shape(B, C, H, W, k, s);
  if (rc) return rc;
  geometry(a, B, C, H, W, k, s);
  const Layout L = layout(a);
  const int ws_rc = check_workspace(ws, ws_bytes, L.total);
  if (ws_rc) return ws_rc;
  char *base = (char *)ws;
  a.x = x;
  a.g = g;
  a.QT = (float *)(base + L.QT);
  a.CT = (float *)(base + L.CT);
  a.pmin = (float *)(base + L.pmin);
  a.pidx = (int *)(base + L.pidx);
  a.part = (double *)(base + L.part);
  a.alpha = alpha;
  a.beta = beta;
  return 0;
}

inline void launch(const Args &a, hipStream_t st) {
  hipLaunchKernelGGL(bbl_pack, dim3((unsigned)(a.nrb + a.ncb), (unsigned)a.B), dim3(NT), 0, st, a);
  const dim3 grid((unsigned)((a.nrb + NT / 64 - 1) / (NT / 64)), (unsigned)a.nsplit, (unsigned)a.B);
  if (a.d + 1 <= 28)
    hipLaunchKernelGGL(bbl_search<14>, grid, dim3(NT), 0, st, a);
  else
    hipLaunchKernelGGL(bbl_search<16>, grid, dim3(NT), 0, st, a);
  hipLaunchKernelGGL(bbl_loss, dim3((unsigned)a.nb3, (unsigned)a.B), dim3(NT), 0, st, a);
  if (a.loss) hipLaunchKernelGGL(bbl_fold, dim3(1), dim3(NT), 0, st, a);
}

}  // namespace bbl
}  // namespace ssg

using namespace ssg::bbl;

extern "C" {

size_t ssg_bbl_workspace_bytes(int B, int C, int H, int W, int k, int stride) {
  if (check_shape(B, C, H, W, k, stride)) return 0;
  Args a{};
  geometry(a, B, C, H, W, k, stride);
  return layout(a).total;
}

int ssg_bbl_search(const float *x, const float *gt, int B, int C, int H, int W, int k, int stride, float alpha,
                   float beta, int *ind_out, float *p1_out, float *sel_out, void *workspace, size_t workspace_bytes,
                   ssg_stream_t stream) {
  if (!x || !gt || !ind_out || !workspace) return SSG_E_BADARG;
  Args a{};
  const int rc = prepare(a, x, gt, B, C, H, W, k, stride, alpha, beta, workspace, workspace_bytes);
  if (rc) return rc;
  a.ind = ind_out;
  a.p1 = p1_out;
  a.sel = sel_out;
  launch(a, (hipStream_t)stream);
  return (int)hipGetLastError();
}

int ssg_bbl_loss(const float *x, const float *gt, int B, int C, int H, int W, int k, int stride, float alpha,
                 float beta, float loss_weight, int mean, float *loss_out, float *grad_x, int *ind_out,
                 void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  if (!x || !gt || !loss_out || !workspace) return SSG_E_BADARG;
  Args a{};
  const int rc = prepare(a, x, gt, B, C, H, W, k, stride, alpha, beta, workspace, workspace_bytes);
  if (rc) return rc;
  a.ind = ind_out;
  a.grad = grad_x;
  a.loss = loss_out;
  a.loss_scale = mean ? (double)loss_weight / ((double)B * a.N * a.d) : (double)loss_weight;
  a.scale = (float)a.loss_scale;
  launch(a, (hipStream_t)stream);
  return (int)hipGetLastError();
}

int ssg_flat_mask(const float *img, int B, int H, int W, int k, float thresh, float *mask_out, ssg_stream_t stream) {
  if (!img || !mask_out || k < 3 || k % 2 == 0 || B <= 0 || H <= 0 || W <= 0) return SSG_E_BADARG;
  if (k > KMAX || B > 65535 || (double)B * 3 * H * W >= 2147483648.0) return SSG_E_TOOLARGE;
  if (H <= k / 2 || W <= k / 2) return SSG_E_IMAGESMALL;
  const int tiles_x = (W + TW - 1) / TW;
  const dim3 grid((unsigned)(tiles_x * ((H + TH - 1) / TH)), (unsigned)B);
  const hipStream_t st = (hipStream_t)stream;
  if (k == 11)
    hipLaunchKernelGGL((flat_mask<11>), grid, dim3(NT), 0, st, img, mask_out, H, W, k, thresh, tiles_x);
  else
    hipLaunchKernelGGL((flat_mask<0>), grid, dim3(NT), 0, st, img, mask_out, H, W, k, thresh, tiles_x);
  return (int)hipGetLastError();
}

}  // extern "C"
