// NIQE, the no-reference metric, on the GPU: basicsr/metrics/niqe.py (estimate_aggd_param :13-38, compute_feature
// :41-65, niqe :68-141, calculate_niqe :145-199) on a BGR image, a model's RGB tensor or a given plane, with
// metric_util.py:32-45 (to_y_channel) and matlab_functions.py:16-178 (imresize at scale 1/2) in between.  One score per
// image; nothing is copied to the host.
//
// Contract (fp64 from the integer plane on; this file is compiled with -ffp-contract=off):
//   plane     convert 0 ('y'): pixel::plane_value with ych (quantise, Y) rounded half to even; convert 1 ('gray'):
//             fl32(fl32(fl32(0.114f b + 0.587f g) + 0.299f r) * 255.0f) on b, g, r = fl32(q / 255.0f), rounded half to even
//             -- OpenCV's DOCUMENTED BGR2GRAY weights; OpenCV itself was never run against this, the formula is pinned
//             by its documentation only.  SSG_NIQE_F32_PLANE: the given fp32 plane, rounded.  `crop` pixels leave every
//             side, then the top-left 96 nbh x 96 nbw (nbh = Hc / 96, nbw = Wc / 96) is kept: plane 1, exact integers.
//   plane 2   MATLAB's antialiased bicubic at exactly 1/2: v = plane1 / 255.0; output o reads inputs 2 o - 3 .. 2 o + 4
//             (symmetric, edge-repeating padding at the border of plane 1) under the 8 weights 0.5 cubic(0.5 (3.5 - t)),
//             taps in index order; rows first, then columns; * 255.0.  Not rounded.
//   MSCN      mu = sum g_ij I, e2 = sum g_ij I^2 over the 7 x 7 window g_ij = exp(-((i-3)^2 + (j-3)^2) / (2 (7/6)^2)) /
//             sum, taps in row-major order, indices clamped at the border of the PLANE ('nearest'); sigma =
//             sqrt(|e2 - mu^2|); n = (I - mu) / (sigma + 1).
//   features  per 96 x 96 (plane 2: 48 x 48) block the maps n and n * roll(n, s), s = (0,1), (1,0), (1,1), (1,-1) (the
//             roll wraps inside the block); per map the six sums {x^2 | x < 0, #x < 0, x^2 | x > 0, #x > 0, |x|, x^2},
//             l = sqrt(mean of x^2 over x < 0), r likewise over x > 0, gh = l / r, rhat = mean|x|^2 / mean x^2, t = rhat
//             (gh^3 + 1)(gh + 1) / (gh^2 + 1)^2; alpha = gam[argmin (r_gam - t)^2] over gam = 0.2 : 0.001 : 10, a tie to
//             the lower index, index 0 for a NaN t (np.argmin's answer); beta_l, beta_r = l, r * sqrt(G(1/alpha) /
//             G(3/alpha)).  Row {alpha, (beta_l + beta_r) / 2, then per shift alpha, (beta_r - beta_l) G(2/alpha) /
//             G(1/alpha), beta_l, beta_r}: 18 values per scale, 36 per block, blocks in column-major order (block column
//             outer).  An empty side (no negative or no positive value) gives NaN as 0 / 0 does.
//   fit       nanmean of the columns; covariance (divisor n - 1) of the rows without a NaN, in row order; S = (cov_pris
//             + cov) / 2; score = sqrt(d' S^-1 d), d = mu_pris - nanmean, by a Cholesky factorisation and one forward
//             substitution (S is positive definite whenever it is finite: DESIGN.md).  Fewer than two NaN-free rows: NaN.
//
// Five launches, no atomics, no tickets, every sum in a fixed order (bit-reproducible); no grid is capped:
//   niqe_plane1    one thread per pixel of plane 1.
//   niqe_plane2    a 16 x 32 tile of plane 2 per workgroup: the 38 x 70 inputs (mirror on the index) / 255 to LDS as
//                  fp64, row pass LDS -> LDS, column pass LDS -> global.  (Two launches, not one: a tile of plane 2 reads
//                  pixels of plane 1 that other workgroups form; it reads them back instead of forming them twice.)
//   niqe_features  grid (2 nblk, B), one workgroup per block and scale, scale 1 first.  The haloed tile (clamp on the
//                  index) -> LDS, the 49-tap moments -> n in LDS, the 30 sums per thread in registers, folded in
//                  pixel::block_sum's order, then 5 threads fit (a bisection on the increasing r_gam table and the
//                  exact argmin among the four entries around it).
//   niqe_fit       one workgroup per image.
//   LDS of niqe_features, all of it dynamic (the base stays 16-byte aligned): tile fp32 [102][103] = 42,024 B (scale 2:
//   fp64 [54][55] = 23,760 B), n fp64 [96][97] = 74,496 B (scale 2: [48][49] = 18,816 B), 30 x 4 + 30 fp64 of sums =
//   1,200 B: 117,720 B per workgroup, the scale-1 size for both scales since they share the launch -- ONE workgroup
//   (4 waves) per CU of 160 KiB.  A 2040 x 1356 image is 588 workgroups of a few tens of microseconds; occupancy is
//   not what limits a metric that runs once per validation image.  Lanes run along the block's columns in every pass: 32
//   consecutive dwords or 32 consecutive fp64 per 32-lane group, conflict-free whatever the stride; the strides are odd
//   (103 dwords, 97 and 55 and 49 fp64) so that a wave's two row segments do not start on the same bank.
//   The r_gam table ({gam, r_gam, G(1/g)/G(3/g), G(2/g)/G(1/g)} x 9,801 fp64, computed on the host with tgamma) is
//   uploaded once per device by the first call there; that call must not be made while its stream is being captured.
#include <math.h>

#include <mutex>

#include "ssg_pixel.hpp"

namespace ssg {
namespace niqe {

using pixel::NT;
using pixel::check_workspace;
using pixel::plane_value;

constexpr int BS = 96;                   // block side on plane 1 (48 on plane 2)
constexpr int R = 3, K = 2 * R + 1;      // the 7 x 7 window
constexpr int NTAB = 9801;               // 0.2 : 0.001 : 10
constexpr int NF = 36;                   // features per block (18 per scale)
constexpr int PT = 8;                    // taps of the 1/2 resize
constexpr int TW2 = 32, TH2 = 16;        // niqe_plane2's output tile
constexpr int IW2 = 2 * TW2 + PT - 2, IH2 = 2 * TH2 + PT - 2;   // 70 x 38 inputs
constexpr int IWS2 = IW2 + 1;            // 71
constexpr int NSUM = 30;                 // 5 maps x 6 sums

struct Args {
  const void *img;
  float *p1;            // (B, H1, W1)
  double *p2;           // (B, H2, W2)
  double *feat;         // (B, nblk, 36)
  int *good;            // (B, nblk): 1 for a row without a NaN
  const double *tab;    // {gam, r_gam, G(1/g)/G(3/g), G(2/g)/G(1/g)} x NTAB
  const double *mu_pris, *cov_pris;
  double *out;          // (B)
  double g[K * K];
  double w[PT];
  int kind, B, C, H, W, crop, convert, ych;
  int nbh, nbw, nblk, H1, W1, H2, W2;
};

// plane-1 value at (y, x) of the UNCROPPED image
__device__ __forceinline__ float niqe_value(const Args &a, int n, int y, int x) {
  if (a.kind == SSG_NIQE_F32_PLANE) return rintf(((const float *)a.img)[((size_t)n * a.H + y) * a.W + x]);
  if (a.convert == 0) return rintf(plane_value(a.img, a, n, 0, y, x));
  // 'gray' (C == 3): a.ych is 0 here, so plane p is the integer q of BGR channel p
  const float b = plane_value(a.img, a, n, 0, y, x) / 255.0f, g = plane_value(a.img, a, n, 1, y, x) / 255.0f,
              r = plane_value(a.img, a, n, 2, y, x) / 255.0f;
  return rintf(((0.114f * b + 0.587f * g) + 0.299f * r) * 255.0f);
}

__global__ __launch_bounds__(NT) void niqe_plane1(Args a) {
  const size_t n = (size_t)a.B * a.H1 * a.W1;
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % a.W1);
  const size_t r = i / a.W1;
  const int y = (int)(r % a.H1), img = (int)(r / a.H1);
  a.p1[i] = niqe_value(a, img, y + a.crop, x + a.crop);
}

// symmetric (edge-repeating) padding; the clamp only serves tile positions beyond plane 2, which are not stored
__device__ __forceinline__ int mirror_clamp(int i, int n) {
  i = i < 0 ? -1 - i : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(NT) void niqe_plane2(Args a) {
  __shared__ double tin[IH2 * IWS2];
  __shared__ double mid[TH2 * IWS2];
  const int ntx = (a.W2 + TW2 - 1) / TW2;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx, img = blockIdx.y;
  const int oy0 = ty * TH2, ox0 = tx * TW2;
  const float *src = a.p1 + (size_t)img * a.H1 * a.W1;
  for (int e = threadIdx.x; e < IH2 * IW2; e += NT) {
    const int ly = e / IW2, lx = e - ly * IW2;
    const int y = mirror_clamp(2 * oy0 - 3 + ly, a.H1), x = mirror_clamp(2 * ox0 - 3 + lx, a.W1);
    tin[ly * IWS2 + lx] = (double)src[(size_t)y * a.W1 + x] / 255.0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TH2 * IW2; e += NT) {
    const int oy = e / IW2, lx = e - oy * IW2;
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < PT; ++t) s += a.w[t] * tin[(2 * oy + t) * IWS2 + lx];
    mid[oy * IWS2 + lx] = s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TH2 * TW2; e += NT) {
    const int oy = e / TW2, ox = e - oy * TW2;
    if (oy0 + oy < a.H2 && ox0 + ox < a.W2) {
      double s = 0.0;
#pragma unroll
      for (int t = 0; t < PT; ++t) s += a.w[t] * mid[oy * IWS2 + 2 * ox + t];
      a.p2[((size_t)img * a.H2 + oy0 + oy) * a.W2 + ox0 + ox] = s * 255.0;
    }
  }
}

// LDS of niqe_features (bytes), the scale-1 sizes
constexpr int TS1 = BS + 2 * R + 1;      // 103: fp32 row stride of the scale-1 tile
constexpr int TILE_BYTES = (BS + 2 * R) * TS1 * 4;          // 42,024 (>= the scale-2 tile's 54 * 55 * 8)
constexpr int N_BYTES = BS * (BS + 1) * 8;                  // 74,496
constexpr int RED_BYTES = (NSUM * (NT / 64) + NSUM) * 8;    // 1,200
constexpr int FEAT_LDS = TILE_BYTES + N_BYTES + RED_BYTES;  // 117,720
static_assert(TILE_BYTES % 8 == 0, "fp64 behind the tile");
static_assert((BS / 2 + 2 * R) * (BS / 2 + 2 * R + 1) * 8 <= TILE_BYTES, "the scale-2 tile fits the scale-1 tile's place");

// one AGGD fit from a map's six sums; returns the table index, *l and *r the one-sided deviations
__device__ __forceinline__ int aggd_index(const double *s, double npix, const double *tab, double *l, double *r) {
  const double left = sqrt(s[0] / s[1]), right = sqrt(s[2] / s[3]);
  const double gh = left / right;
  const double ma = s[4] / npix;
  const double rhat = (ma * ma) / (s[5] / npix);
  const double gh2 = gh * gh;
  const double t = (rhat * (gh2 * gh + 1.0) * (gh + 1.0)) / ((gh2 + 1.0) * (gh2 + 1.0));
  *l = left;
  *r = right;
  if (!(t == t)) return 0;              // np.argmin of an all-NaN array
  const double *rg = tab + NTAB;
  int lo = 0, hi = NTAB;                // the first index with rg >= t
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (rg[m] < t) lo = m + 1; else hi = m;
  }
  int best = max(lo - 2, 0);
  double bd = (rg[best] - t) * (rg[best] - t);
  for (int i = best + 1; i <= min(lo + 1, NTAB - 1); ++i) {
    const double d = (rg[i] - t) * (rg[i] - t);
    if (d < bd) bd = d, best = i;       // a tie keeps the lower index
  }
  return best;
}

template <class T, int S>   // S: block side
__device__ __forceinline__ void block_features(const Args &a, const T *plane, int PH, int PW, int by, int bx,
                                               double *row, char *lds) {
  constexpr int TWD = S + 2 * R, TS = TWD + 1, NS = S + 1;
  T *tile = (T *)lds;
  double *nm = (double *)(lds + TILE_BYTES);
  double *red = (double *)(lds + TILE_BYTES + N_BYTES);     // [NSUM][NT / 64]
  double *tot = red + NSUM * (NT / 64);                     // [NSUM]
  const int y0 = by * S - R, x0 = bx * S - R;
  for (int e = threadIdx.x; e < TWD * TWD; e += NT) {
    const int ly = e / TWD, lx = e - ly * TWD;
    const int y = min(max(y0 + ly, 0), PH - 1), x = min(max(x0 + lx, 0), PW - 1);
    tile[ly * TS + lx] = plane[(size_t)y * PW + x];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < S * S; e += NT) {
    const int y = e / S, x = e - y * S;
    const T *c = tile + y * TS + x;
    double mu = 0.0, e2 = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double v = (double)c[i * TS + j], w = a.g[i * K + j];
        mu += w * v;
        e2 += w * (v * v);
      }
    const double sigma = sqrt(fabs(e2 - mu * mu));
    nm[y * NS + x] = ((double)c[R * TS + R] - mu) / (sigma + 1.0);
  }
  __syncthreads();
  double acc[NSUM];
#pragma unroll
  for (int q = 0; q < NSUM; ++q) acc[q] = 0.0;
  for (int e = threadIdx.x; e < S * S; e += NT) {
    const int y = e / S, x = e - y * S;
    const int ym = y == 0 ? S - 1 : y - 1, xm = x == 0 ? S - 1 : x - 1, xp = x == S - 1 ? 0 : x + 1;
    const double v = nm[y * NS + x];
    double m[5];
    m[0] = v;
    m[1] = v * nm[y * NS + xm];
    m[2] = v * nm[ym * NS + x];
    m[3] = v * nm[ym * NS + xm];
    m[4] = v * nm[ym * NS + xp];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double u = m[k], sq = u * u;
      if (u < 0.0) {
        acc[k * 6 + 0] += sq;
        acc[k * 6 + 1] += 1.0;
      } else if (u > 0.0) {
        acc[k * 6 + 2] += sq;
        acc[k * 6 + 3] += 1.0;
      }
      acc[k * 6 + 4] += fabs(u);
      acc[k * 6 + 5] += sq;
    }
  }
  // the 30 sums in pixel::block_sum's order: the wave's lanes by halving, then the waves in index order
#pragma unroll
  for (int q = 0; q < NSUM; ++q) {
    double v = acc[q];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) red[q * (NT / 64) + (threadIdx.x >> 6)] = v;
  }
  __syncthreads();
  if (threadIdx.x < NSUM) {
    double s = red[threadIdx.x * (NT / 64)];
    for (int i = 1; i < NT / 64; ++i) s += red[threadIdx.x * (NT / 64) + i];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    double l, r;
    const int idx = aggd_index(tot + k * 6, (double)(S * S), a.tab, &l, &r);
    const double alpha = a.tab[idx], sc = sqrt(a.tab[2 * NTAB + idx]);
    const double bl = l * sc, br = r * sc;
    if (k == 0) {
      row[0] = alpha;
      row[1] = (bl + br) / 2.0;
    } else {
      double *o = row + 2 + 4 * (k - 1);
      o[0] = alpha;
      o[1] = (br - bl) * a.tab[3 * NTAB + idx];
      o[2] = bl;
      o[3] = br;
    }
  }
}

__global__ __launch_bounds__(NT) void niqe_features(Args a) {
  extern __shared__ __attribute__((aligned(16))) char niqe_lds[];
  const int img = blockIdx.y;
  const int scale2 = (int)blockIdx.x >= a.nblk;
  const int blk = (int)blockIdx.x - (scale2 ? a.nblk : 0);
  const int bx = blk / a.nbh, by = blk - bx * a.nbh;        // rows in column-major block order
  double *row = a.feat + ((size_t)img * a.nblk + blk) * NF + (scale2 ? NF / 2 : 0);
  if (!scale2)
    block_features<float, BS>(a, a.p1 + (size_t)img * a.H1 * a.W1, a.H1, a.W1, by, bx, row, niqe_lds);
  else
    block_features<double, BS / 2>(a, a.p2 + (size_t)img * a.H2 * a.W2, a.H2, a.W2, by, bx, row, niqe_lds);
}

constexpr int FL = 7;                    // niqe_fit: row lanes per column (36 x 7 = 252 threads)
constexpr int SS = NF + 1;               // 37: row stride of S

__global__ __launch_bounds__(NT) void niqe_fit(Args a) {
  __shared__ double S[NF * SS];
  __shared__ double ps[FL * NF], pg[FL * NF];
  __shared__ int pc[FL * NF];
  __shared__ double cmean[NF], gmean[NF], y[NF];
  __shared__ int wave_good[NT / 64];
  const int img = blockIdx.x, tid = threadIdx.x;
  const double *feat = a.feat + (size_t)img * a.nblk * NF;
  int *good = a.good + (size_t)img * a.nblk;
  // ---- the rows without a NaN ----
  int mine = 0;
  for (int r = tid; r < a.nblk; r += NT) {
    int ok = 1;
    for (int c = 0; c < NF; ++c) {
      const double v = feat[(size_t)r * NF + c];
      ok &= (v == v);
    }
    good[r] = ok;
    mine += ok;
  }
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
  if ((tid & 63) == 0) wave_good[tid >> 6] = mine;
  __syncthreads();   // (also: good[] is visible to the whole workgroup)
  int ngood = 0;
  for (int i = 0; i < NT / 64; ++i) ngood += wave_good[i];
  // ---- column means: over the non-NaN entries (nanmean), and over the NaN-free rows (the covariance's centre) ----
  if (tid < FL * NF) {
    const int l = tid / NF, c = tid - l * NF;
    double s = 0.0, gs = 0.0;
    int cnt = 0;
    for (int r = l; r < a.nblk; r += FL) {
      const double v = feat[(size_t)r * NF + c];
      if (v == v) s += v, ++cnt;
      if (good[r]) gs += v;
    }
    ps[tid] = s, pg[tid] = gs, pc[tid] = cnt;
  }
  __syncthreads();
  if (tid < NF) {
    double s = 0.0, gs = 0.0;
    int cnt = 0;
    for (int l = 0; l < FL; ++l) s += ps[l * NF + tid], gs += pg[l * NF + tid], cnt += pc[l * NF + tid];
    cmean[tid] = s / (double)cnt;
    gmean[tid] = gs / (double)ngood;
  }
  __syncthreads();
  // ---- S = (cov_pris + cov) / 2, the lower triangle; every entry sums its rows in index order ----
  for (int e = tid; e < NF * NF; e += NT) {
    const int i = e / NF, j = e - i * NF;
    if (j > i) continue;
    const double mi = gmean[i], mj = gmean[j];
    double s = 0.0;
    for (int r = 0; r < a.nblk; ++r)
      if (good[r]) s += (feat[(size_t)r * NF + i] - mi) * (feat[(size_t)r * NF + j] - mj);
    const double cov = ngood >= 2 ? s / (double)(ngood - 1) : (double)NAN;
    S[i * SS + j] = (a.cov_pris[i * NF + j] + cov) / 2.0;
  }
  __syncthreads();
  // ---- Cholesky, right-looking: column k, then the trailing update; a non-positive pivot ends in NaN ----
  for (int k = 0; k < NF; ++k) {
    if (tid == 0) S[k * SS + k] = sqrt(S[k * SS + k]);
    __syncthreads();
    if (tid > k && tid < NF) S[tid * SS + k] /= S[k * SS + k];
    __syncthreads();
    for (int e = tid; e < NF * NF; e += NT) {
      const int i = e / NF, j = e - i * NF;
      if (j > k && j <= i) S[i * SS + j] -= S[i * SS + k] * S[j * SS + k];
    }
    __syncthreads();
  }
  // ---- L y = d; score = |y| ----
  if (tid == 0) {
    double q = 0.0;
    for (int i = 0; i < NF; ++i) {
      double s = a.mu_pris[i] - cmean[i];
      for (int j = 0; j < i; ++j) s -= S[i * SS + j] * y[j];
      y[i] = s / S[i * SS + i];
      q += y[i] * y[i];
    }
    a.out[img] = sqrt(q);
  }
}

// ---------------------------------------------------------------------------------------------------------- host ---
struct Table {
  double v[4 * NTAB];
  Table() {
    const double first = 0.2, delta = (0.2 + 0.001) - 0.2;   // np.arange's own arithmetic: first + i * (second - first)
    for (int i = 0; i < NTAB; ++i) {
      const double g = first + (double)i * delta, rec = 1.0 / g;
      const double g2 = tgamma(rec * 2.0);
      v[i] = g;
      v[NTAB + i] = (g2 * g2) / (tgamma(rec) * tgamma(rec * 3.0));
      v[2 * NTAB + i] = tgamma(1.0 / g) / tgamma(3.0 / g);
      v[3 * NTAB + i] = tgamma(2.0 / g) / tgamma(1.0 / g);
    }
  }
};

inline const Table &host_table() {
  static const Table t;
  return t;
}

// the device's copy, uploaded by the first call on that device
inline int device_table(const double **out) {
  constexpr int MAXDEV = 64;
  static std::mutex mu;
  static double *tab[MAXDEV] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  if (dev < 0 || dev >= MAXDEV) return SSG_E_TOOLARGE;
  std::lock_guard<std::mutex> lk(mu);
  if (!tab[dev]) {
    double *d = nullptr;
    e = hipMalloc(&d, sizeof(double) * 4 * NTAB);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(d, host_table().v, sizeof(double) * 4 * NTAB, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return (int)e;
    }
    tab[dev] = d;
  }
  *out = tab[dev];
  return 0;
}

inline int check_shape(int kind, int B, int C, int H, int W, int crop, int convert) {
  if (B <= 0 || H <= 0 || W <= 0 || crop < 0) return SSG_E_BADARG;
  if (C != 1 && C != 3) return SSG_E_BADARG;
  if (kind != SSG_METRIC_F32_RGB && kind != SSG_METRIC_U8_HWC && kind != SSG_METRIC_U8_CHW && kind != SSG_NIQE_F32_PLANE)
    return SSG_E_BADARG;
  if (kind == SSG_NIQE_F32_PLANE && C != 1) return SSG_E_BADARG;
  if (convert != 0 && convert != 1) return SSG_E_BADARG;
  if (convert == 1 && C != 3 && kind != SSG_NIQE_F32_PLANE) return SSG_E_BADARG;   // (OpenCV's BGR2GRAY takes 3 channels)
  if (B > 65535 || (double)B * C * H * W >= 2147483648.0) return SSG_E_TOOLARGE;
  if ((long)H - 2L * crop < BS || (long)W - 2L * crop < BS) return SSG_E_IMAGESMALL;
  return 0;
}

inline void geometry(Args &a, int kind, int B, int C, int H, int W, int crop, int convert) {
  a.kind = kind, a.B = B, a.C = C, a.H = H, a.W = W, a.crop = crop, a.convert = convert;
  a.ych = convert == 0;                 // what pixel::plane_value reads
  a.nbh = (H - 2 * crop) / BS, a.nbw = (W - 2 * crop) / BS;
  a.nblk = a.nbh * a.nbw;
  a.H1 = a.nbh * BS, a.W1 = a.nbw * BS;
  a.H2 = a.H1 / 2, a.W2 = a.W1 / 2;
  const double sigma = 7.0 / 6.0;
  double sum = 0.0;
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j)
      sum += a.g[i * K + j] = exp(-(double)((i - R) * (i - R) + (j - R) * (j - R)) / (2.0 * sigma * sigma));
  for (int i = 0; i < K * K; ++i) a.g[i] /= sum;
  // Keys' cubic (a = -0.5) stretched by 2: tap t lies 3.5 - t input pixels from the output's centre
  sum = 0.0;
  for (int t = 0; t < PT; ++t) {
    const double x = fabs(0.5 * (3.5 - t)), x2 = x * x, x3 = x2 * x;
    sum += a.w[t] = 0.5 * (x <= 1.0 ? 1.5 * x3 - 2.5 * x2 + 1.0 : -0.5 * x3 + 2.5 * x2 - 4.0 * x + 2.0);
  }
  for (int t = 0; t < PT; ++t) a.w[t] /= sum;
}

struct Layout {
  size_t p1, p2, feat, good, total;
};

inline Layout layout(const Args &a) {
  Layout L;
  Carver c;
  L.p1 = c.take(sizeof(float) * (size_t)a.B * a.H1 * a.W1);
  L.p2 = c.take(sizeof(double) * (size_t)a.B * a.H2 * a.W2);
  L.feat = c.take(sizeof(double) * (size_t)a.B * a.nblk * NF);
  L.good = c.take(sizeof(int) * (size_t)a.B * a.nblk);
  L.total = c.end;
  return L;
}

inline void launch_planes(const Args &a, hipStream_t st) {
  const size_t n = (size_t)a.B * a.H1 * a.W1;             // < 2^31
  hipLaunchKernelGGL(niqe_plane1, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, a);
  const int tiles = ((a.W2 + TW2 - 1) / TW2) * ((a.H2 + TH2 - 1) / TH2);
  hipLaunchKernelGGL(niqe_plane2, dim3((unsigned)tiles, (unsigned)a.B), dim3(NT), 0, st, a);
}

inline int launch_features(const Args &a, hipStream_t st) {
  static std::atomic<unsigned long long> lds_set{0};
  if (const int rc = ensure_dynamic_lds(niqe_features, FEAT_LDS, lds_set)) return rc;
  hipLaunchKernelGGL(niqe_features, dim3((unsigned)(2 * a.nblk), (unsigned)a.B), dim3(NT), FEAT_LDS, st, a);
  return 0;
}

// the checks and the carving shared by ssg_niqe and ssg_niqe_features
inline int prepare(Args &a, const void *img, int kind, int B, int C, int H, int W, int crop, int convert, void *ws,
                   size_t ws_bytes) {
  const int rc = check_shape(kind, B, C, H, W, crop, convert);
  if (rc) return rc;
  geometry(a, kind, B, C, H, W, crop, convert);
  const Layout L = layout(a);
  const int ws_rc = check_workspace(ws, ws_bytes, L.total);
  if (ws_rc) return ws_rc;
  a.img = img;
  a.p1 = (float *)((char *)ws + L.p1);
  a.p2 = (double *)((char *)ws + L.p2);
  a.feat = (double *)((char *)ws + L.feat);
  a.good = (int *)((char *)ws + L.good);
  return device_table(&a.tab);
}

}  // namespace niqe
}  // namespace ssg

using namespace ssg::niqe;

extern "C" {

size_t ssg_niqe_workspace_bytes(int B, int C, int H, int W, int crop_border) {
  // (kind and convert do not enter the size: the plane kind has C = 1, like a grey image)
  if (check_shape(C == 1 ? SSG_NIQE_F32_PLANE : SSG_METRIC_F32_RGB, B, C, H, W, crop_border, 0)) return 0;
  Args a{};
  geometry(a, SSG_METRIC_F32_RGB, B, C, H, W, crop_border, 0);
  return layout(a).total;
}

int ssg_niqe_table(double *table_out) {
  if (!table_out) return SSG_E_BADARG;
  const Table &t = host_table();
  for (int i = 0; i < 4 * NTAB; ++i) table_out[i] = t.v[i];
  return 0;
}

int ssg_niqe_planes(const void *img, int kind, int B, int C, int H, int W, int crop_border, int convert, float *plane1,
                    double *plane2, ssg_stream_t stream) {
  if (!img || !plane1 || !plane2) return SSG_E_BADARG;
  const int rc = check_shape(kind, B, C, H, W, crop_border, convert);
  if (rc) return rc;
  Args a{};
  geometry(a, kind, B, C, H, W, crop_border, convert);
  a.img = img;
  a.p1 = plane1;
  a.p2 = plane2;
  launch_planes(a, (hipStream_t)stream);
  return (int)hipGetLastError();
}

int ssg_niqe_features(const void *img, int kind, int B, int C, int H, int W, int crop_border, int convert, double *feat,
                      void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  if (!img || !feat || !workspace) return SSG_E_BADARG;
  Args a{};
  const int rc = prepare(a, img, kind, B, C, H, W, crop_border, convert, workspace, workspace_bytes);
  if (rc) return rc;
  a.feat = feat;
  launch_planes(a, (hipStream_t)stream);
  const int lrc = launch_features(a, (hipStream_t)stream);
  return lrc ? lrc : (int)hipGetLastError();
}

int ssg_niqe(const void *img, int kind, int B, int C, int H, int W, int crop_border, int convert, const double *mu_pris,
             const double *cov_pris, double *out, void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  if (!img || !mu_pris || !cov_pris || !out || !workspace) return SSG_E_BADARG;
  Args a{};
  const int rc = prepare(a, img, kind, B, C, H, W, crop_border, convert, workspace, workspace_bytes);
  if (rc) return rc;
  a.mu_pris = mu_pris;
  a.cov_pris = cov_pris;
  a.out = out;
  launch_planes(a, (hipStream_t)stream);
  const int lrc = launch_features(a, (hipStream_t)stream);
  if (lrc) return lrc;
  hipLaunchKernelGGL(niqe_fit, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
