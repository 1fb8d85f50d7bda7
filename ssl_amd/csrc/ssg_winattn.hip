// SwinIR's (shifted-)window attention between a block's qkv and proj Linears, forward and backward, one launch each:
// GAN-Based-SR/basicsr/archs/swinir_arch.py's torch.roll, window_partition, the qkv permute, q * scale, q k^T, the
// relative-position bias, the shift mask, softmax, attn v, the transpose, window_reverse and the roll back.  Window 8
// (N = 64 tokens), head_dim <= 32.
//
// Contract (this file is compiled with -ffp-contract=off; every fma below is written out).
//   qkv (B, H, W, 3 C) fp32, C = heads head_dim: the qkv Linear applied to the UNPARTITIONED token grid, element
//   [b, y, x, (s heads + h) head_dim + c] for s = 0, 1, 2 (q, k, v).  out, dout (B, H, W, C); dqkv as qkv.
//   A unit is one (image, window, head).  Token (iy, ix) of window (wy, wx) has the shifted coordinate
//   ys = 8 wy + iy, xs = 8 wx + ix and is read from AND written back to ((ys + shift) mod H, (xs + shift) mod W): the
//   two rolls, the partition and the merge are this index arithmetic.
//     qs_i   = fl(q_i scale)                                      per element
//     S_ij   = fma chain over c = 0 .. head_dim - 1 of qs_ic k_jc, from 0     (what the fp32 MFMA computes)
//            + table[(iy_i - iy_j + 7) 15 + (ix_i - ix_j + 7), h]
//            + (shift > 0 ? (label_i != label_j ? -100 : 0) : nothing)
//              label = 3 ly + lx, ly = (ys >= H - 8) + (ys >= H - shift), lx likewise: the reference's calculate_mask
//     P_ij   = expf(S_ij - max_j S_ij) / sum_j expf(..)
//              the sum: thread q of a row's four adds j = q, q + 4, ... ascending, then (t0 + t1) + (t2 + t3)
//     O_ic   = fma chain over j = 0 .. 63 of P_ij v_jc, from 0
//   backward, P recomputed by the same lines (nothing of size N^2 is kept between the calls):
//     dP_ij = fma chain over c of dO_ic v_jc     D_i = sum_j fl(P_ij dP_ij), in the order of the softmax sum
//     dS_ij = fl(P_ij fl(dP_ij - D_i))
//     dv_jc = fma chain over i of P_ij dO_ic     dk_jc = fma chain over i of dS_ij qs_ic
//     dq_ic = fl(scale chain over j of dS_ij k_jc)
//     dtable[idx, h] = sum over the units of head h and the pairs (i, j) of idx of dS_ij, in fp64: a thread adds the
//       pairs of its idx by ascending i within a unit and its workgroup's units in order; a workgroup has ONE head
//       (the grid is a multiple of heads) and writes 225 fp64 partials; a second launch adds a head's partials by
//       ascending workgroup and rounds once.
// One writer per element of out, dqkv, the partials and dtable: no atomics, no tickets, no zero-fill.  A unit reads
// only its window's tokens: the same bits for an image alone or in a batch, wherever it lies, and a NaN stays inside
// its window (in out and dqkv; dtable sums over every window).  Every global access is a 4-byte access at a float's
// alignment.  No scratch.
// Layout: one workgroup of 256 threads per unit, thread (i = tid / 4, q = tid % 4) owns row i's columns q, q + 4, ...
// of S and channels q, q + 4, ... of the row's outputs; q~, k, v (and dO) sit in LDS as [64][33], P / dS as [64][65].
// Grids are capped and walk grid-stride.  This file defines the entry points ssg_winattn_* at its end.
#include "ssg_stream.hpp"

namespace ssg {
namespace wa {

using stream::NT;

constexpr int WS = 8;                    // the window's side
constexpr int N = WS * WS;               // tokens of a window: a wave's lanes
constexpr int DP = 32;                   // head_dim padded (zeros change no chain)
constexpr int LD = DP + 1;               // a tile's row in LDS: 16 rows of a wave meet 16 banks
constexpr int LP = N + 1;                // a row of P
constexpr int NB = (2 * WS - 1) * (2 * WS - 1);   // 225 rows of the bias table
constexpr int PER = N / 4;               // columns of S per thread
constexpr int CH = DP / 4;               // channels of a row per thread
constexpr int GRID_CAP = stream::MAX_WG;
constexpr float MASKED = -100.0f;

struct Shape {
  int H, W, heads, D, shift;
  float scale;
  size_t units;
};

struct Unit {
  size_t image;   // pixels in front of the unit's image: b H W
  int h, y0, x0;  // the head, the window's first shifted row and column
};

__device__ __forceinline__ Unit unit_of(const Shape &s, size_t u) {
  Unit n;
  n.h = (int)(u % (size_t)s.heads);
  const size_t win = u / (size_t)s.heads, nwx = (size_t)(s.W / WS), nwy = (size_t)(s.H / WS);
  n.x0 = (int)(win % nwx) * WS;
  const size_t r = win / nwx;
  n.y0 = (int)(r % nwy) * WS;
  n.image = (r / nwy) * (size_t)s.H * (size_t)s.W;
  return n;
}

// what the first 64 threads and the first 225 prepare for a unit: each token's source pixel and mask label, the head's
// column of the table
__device__ __forceinline__ void prepare(const Shape &s, const Unit &n, const float *table, int *pix, int *label,
                                        float *bias) {
  const int t = threadIdx.x;
  if (t < N) {
    const int ys = n.y0 + (t >> 3), xs = n.x0 + (t & 7);
    int sy = ys + s.shift, sx = xs + s.shift;
    sy = sy >= s.H ? sy - s.H : sy;
    sx = sx >= s.W ? sx - s.W : sx;
    pix[t] = sy * s.W + sx;
    const int ly = (ys >= s.H - WS) + (ys >= s.H - s.shift), lx = (xs >= s.W - WS) + (xs >= s.W - s.shift);
    label[t] = 3 * ly + lx;
  }
  if (t < NB) bias[t] = table[(size_t)t * (size_t)s.heads + (size_t)n.h];
}

// a [64][head_dim] slice of the unit's tokens into LDS, columns head_dim .. 31 zero; 32 lanes per token
template <bool SCALE>
__device__ __forceinline__ void load_tile(float (*dst)[LD], const float *src, size_t row, size_t col, int D,
                                          const int *pix, float scale) {
  for (int e = threadIdx.x; e < N * DP; e += NT) {
    const int tok = e >> 5, c = e & 31;
    float v = 0.0f;
    if (c < D) v = src[(size_t)pix[tok] * row + col + (size_t)c];
    dst[tok][c] = SCALE ? v * scale : v;
  }
}

__device__ __forceinline__ void store_tile(float *dst, const float (*src)[LD], size_t row, size_t col, int D,
                                           const int *pix) {
  for (int e = threadIdx.x; e < N * DP; e += NT) {
    const int tok = e >> 5, c = e & 31;
    if (c < D) dst[(size_t)pix[tok] * row + col + (size_t)c] = src[tok][c];
  }
}

// the sum of a row's 64 values held 16 per thread by its four threads: each thread ascending, then (t0 + t1) + (t2 + t3)
__device__ __forceinline__ float row_sum(const float (&v)[PER]) {
  float t = v[0];
#pragma unroll
  for (int k = 1; k < PER; ++k) t = t + v[k];
  t = t + __shfl_xor(t, 1, 64);
  t = t + __shfl_xor(t, 2, 64);
  return t;
}

// thread (i, q): P_ij for j = q + 4 k
__device__ __forceinline__ void softmax_row(const float (*Q)[LD], const float (*K)[LD], const float *bias,
                                            const int *label, bool masked, int D, int i, int q, float (&p)[PER]) {
#pragma unroll
  for (int k = 0; k < PER; ++k) p[k] = 0.0f;
  for (int c = 0; c < D; ++c) {
    const float qv = Q[i][c];
#pragma unroll
    for (int k = 0; k < PER; ++k) p[k] = fmaf(qv, K[q + 4 * k][c], p[k]);
  }
  const int iy = i >> 3, ix = i & 7, li = label[i];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int j = q + 4 * k;
    float sc = p[k] + bias[(iy - (j >> 3) + WS - 1) * (2 * WS - 1) + (ix - (j & 7) + WS - 1)];
    if (masked) sc = sc + (label[j] != li ? MASKED : 0.0f);
    p[k] = sc;
  }
  float m = p[0];
#pragma unroll
  for (int k = 1; k < PER; ++k) m = fmaxf(m, p[k]);
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
#pragma unroll
  for (int k = 0; k < PER; ++k) p[k] = expf(p[k] - m);
  const float den = row_sum(p);
#pragma unroll
  for (int k = 0; k < PER; ++k) p[k] = p[k] / den;
}

// acc_c = fma chain over r = 0 .. 63 of X[r][col] T[r][q + 4 c] (ROWS: X[col][r] T[r][..]): the three products whose
// sum runs over a whole row or column of P / dS
template <bool ROWS>
__device__ __forceinline__ void chain64(const float (*X)[LP], const float (*T)[LD], int col, int q, float (&acc)[CH]) {
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c] = 0.0f;
#pragma unroll 4
  for (int r = 0; r < N; ++r) {
    const float x = ROWS ? X[col][r] : X[r][col];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = fmaf(x, T[r][q + 4 * c], acc[c]);
  }
}

__global__ __launch_bounds__(NT) void winattn_fwd_kernel(const float *qkv, const float *table, float *out, Shape s) {
  __shared__ float Q[N][LD], K[N][LD], V[N][LD], P[N][LP], bias[NB];
  __shared__ int pix[N], label[N];
  const int i = threadIdx.x >> 2, q = threadIdx.x & 3;
  const size_t C = (size_t)s.heads * (size_t)s.D;
  for (size_t u = blockIdx.x; u < s.units; u += gridDim.x) {
    const Unit n = unit_of(s, u);
    prepare(s, n, table, pix, label, bias);
    __syncthreads();
    const float *src = qkv + n.image * 3 * C;
    const size_t col = (size_t)n.h * (size_t)s.D;
    load_tile<true>(Q, src, 3 * C, col, s.D, pix, s.scale);
    load_tile<false>(K, src, 3 * C, C + col, s.D, pix, 0.0f);
    load_tile<false>(V, src, 3 * C, 2 * C + col, s.D, pix, 0.0f);
    __syncthreads();
    float p[PER];
    softmax_row(Q, K, bias, label, s.shift > 0, s.D, i, q, p);
#pragma unroll
    for (int k = 0; k < PER; ++k) P[i][q + 4 * k] = p[k];
    __syncthreads();                       // (every thread is done with Q and K)
    float o[CH];
    chain64<true>(P, V, i, q, o);
#pragma unroll
    for (int c = 0; c < CH; ++c) Q[i][q + 4 * c] = o[c];
    __syncthreads();
    store_tile(out + n.image * C, Q, C, col, s.D, pix);
    __syncthreads();
  }
}

__global__ __launch_bounds__(NT) void winattn_bwd_kernel(const float *qkv, const float *table, const float *dout,
                                                         float *dqkv, double *part, Shape s) {
  __shared__ float Q[N][LD], K[N][LD], V[N][LD], G[N][LD], X[N][LP], bias[NB];
  __shared__ int pix[N], label[N];
  const int t = threadIdx.x, i = t >> 2, q = t & 3;
  const size_t C = (size_t)s.heads * (size_t)s.D;
  double table_sum = 0.0;                  // thread t < 225: row t of this workgroup's head, over its units
  for (size_t u = blockIdx.x; u < s.units; u += gridDim.x) {
    const Unit n = unit_of(s, u);
    prepare(s, n, table, pix, label, bias);
    __syncthreads();
    const float *src = qkv + n.image * 3 * C;
    const size_t col = (size_t)n.h * (size_t)s.D;
    load_tile<true>(Q, src, 3 * C, col, s.D, pix, s.scale);
    load_tile<false>(K, src, 3 * C, C + col, s.D, pix, 0.0f);
    load_tile<false>(V, src, 3 * C, 2 * C + col, s.D, pix, 0.0f);
    load_tile<false>(G, dout + n.image * C, C, col, s.D, pix, 0.0f);
    __syncthreads();
    float p[PER], ds[PER];
    softmax_row(Q, K, bias, label, s.shift > 0, s.D, i, q, p);
#pragma unroll
    for (int k = 0; k < PER; ++k) ds[k] = 0.0f;
    for (int c = 0; c < s.D; ++c) {
      const float g = G[i][c];
#pragma unroll
      for (int k = 0; k < PER; ++k) ds[k] = fmaf(g, V[q + 4 * k][c], ds[k]);
    }
    {
      float pd[PER];
#pragma unroll
      for (int k = 0; k < PER; ++k) pd[k] = p[k] * ds[k];
      const float D = row_sum(pd);
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const float diff = ds[k] - D;
        ds[k] = p[k] * diff;
      }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) X[i][q + 4 * k] = p[k];
    __syncthreads();                       // X = P; every thread is done with V
    float a[CH], b[CH];
    chain64<false>(X, G, i, q, a);         // dv of token i
#pragma unroll
    for (int c = 0; c < CH; ++c) V[i][q + 4 * c] = a[c];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) X[i][q + 4 * k] = ds[k];
    __syncthreads();                       // X = dS
    chain64<true>(X, K, i, q, a);          // dq of token i, before the scale
    chain64<false>(X, Q, i, q, b);         // dk of token i
    if (part && t < NB) {
      const int dy = t / (2 * WS - 1) - (WS - 1), dx = t % (2 * WS - 1) - (WS - 1);
      const int y_lo = dy > 0 ? dy : 0, y_hi = dy > 0 ? WS : WS + dy, x_lo = dx > 0 ? dx : 0, x_hi = dx > 0 ? WS : WS + dx;
      for (int y = y_lo; y < y_hi; ++y)
        for (int x = x_lo; x < x_hi; ++x) table_sum += (double)X[y * WS + x][(y - dy) * WS + (x - dx)];
    }
    __syncthreads();                       // every thread is done with Q, K and X
#pragma unroll
    for (int c = 0; c < CH; ++c) Q[i][q + 4 * c] = s.scale * a[c], K[i][q + 4 * c] = b[c];
    __syncthreads();
    float *dst = dqkv + n.image * 3 * C;
    store_tile(dst, Q, 3 * C, col, s.D, pix);
    store_tile(dst, K, 3 * C, C + col, s.D, pix);
    store_tile(dst, V, 3 * C, 2 * C + col, s.D, pix);
    __syncthreads();
  }
  if (part && t < NB) part[(size_t)blockIdx.x * NB + t] = table_sum;
}

// workgroup h: dtable[., h] from the partials of the workgroups h, h + heads, ... in that order
__global__ __launch_bounds__(NT) void winattn_table_kernel(const double *part, float *dtable, int heads, unsigned grid) {
  const unsigned h = blockIdx.x, t = threadIdx.x;
  if (t >= NB) return;
  double sum = 0.0;
  for (size_t g = h; g < grid; g += (size_t)heads) sum += part[g * NB + t];
  dtable[(size_t)t * (size_t)heads + h] = (float)sum;
}

// ---- host ----
// 0, or why the shape cannot be launched
static int refuse_shape(int B, int H, int W, int heads, int head_dim, int shift) {
  if (B < 1 || H < 1 || W < 1 || heads < 1) return SSG_E_BADARG;
  if (H % WS || W % WS || shift < 0 || shift >= WS || head_dim < 1 || head_dim > DP) return SSG_E_BADARG;
  if ((size_t)H * (size_t)W > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  const size_t windows = (size_t)B * (size_t)(H / WS) * (size_t)(W / WS);
  if (windows > (size_t)INT_MAX / (size_t)heads) return SSG_E_TOOLARGE;
  return 0;
}

static size_t units_of(int B, int H, int W, int heads) {
  return (size_t)B * (size_t)(H / WS) * (size_t)(W / WS) * (size_t)heads;
}

// one workgroup per unit under the cap, and a multiple of heads: a workgroup then keeps its head from trip to trip
static unsigned grid_of(size_t units, int heads) {
  const size_t cap = (size_t)heads > (size_t)GRID_CAP ? (size_t)heads : (size_t)(GRID_CAP - GRID_CAP % heads);
  return (unsigned)(units < cap ? units : cap);
}

static Shape shape_of(int B, int H, int W, int heads, int head_dim, int shift, float scale) {
  return Shape{H, W, heads, head_dim, shift, scale, units_of(B, H, W, heads)};
}

}  // namespace wa
}  // namespace ssg

// ---- (Z) the entry points: every refusal is decided here, before any launch ----
using namespace ssg;

extern "C" {

int ssg_winattn_grid_cap(void) { return wa::GRID_CAP; }

size_t ssg_winattn_workspace_bytes(int B, int H, int W, int heads, int head_dim) {
  if (wa::refuse_shape(B, H, W, heads, head_dim, 0)) return 0;
  return sizeof(double) * wa::NB * (size_t)wa::grid_of(wa::units_of(B, H, W, heads), heads);
}

int ssg_winattn_forward(const float *qkv, const float *bias_table, float *out, int B, int H, int W, int heads,
                        int head_dim, int shift, float scale, ssg_stream_t stream) {
  using namespace wa;
  if (!qkv || !bias_table || !out) return SSG_E_BADARG;
  if (const int rc = refuse_shape(B, H, W, heads, head_dim, shift)) return rc;
  if (unaligned(qkv, sizeof(float)) || unaligned(bias_table, sizeof(float)) || unaligned(out, sizeof(float)))
    return SSG_E_ALIGN;
  const Shape s = shape_of(B, H, W, heads, head_dim, shift, scale);
  hipLaunchKernelGGL(winattn_fwd_kernel, dim3(grid_of(s.units, heads)), dim3(NT), 0, (hipStream_t)stream, qkv,
                     bias_table, out, s);
  return (int)hipGetLastError();
}

int ssg_winattn_backward(const float *qkv, const float *bias_table, const float *dout, float *dqkv, float *dbias_table,
                         void *workspace, size_t workspace_bytes, int B, int H, int W, int heads, int head_dim,
                         int shift, float scale, ssg_stream_t stream) {
  using namespace wa;
  if (!qkv || !bias_table || !dout || !dqkv || (dbias_table && !workspace)) return SSG_E_BADARG;
  if (const int rc = refuse_shape(B, H, W, heads, head_dim, shift)) return rc;
  if (unaligned(qkv, sizeof(float)) || unaligned(bias_table, sizeof(float)) || unaligned(dout, sizeof(float)) ||
      unaligned(dqkv, sizeof(float)) || unaligned(dbias_table, sizeof(float)) ||
      (dbias_table && unaligned(workspace, sizeof(double))))
    return SSG_E_ALIGN;
  if (dbias_table && workspace_bytes < ssg_winattn_workspace_bytes(B, H, W, heads, head_dim)) return SSG_E_WORKSPACE;
  const Shape s = shape_of(B, H, W, heads, head_dim, shift, scale);
  const unsigned grid = grid_of(s.units, heads);
  const hipStream_t st = (hipStream_t)stream;
  double *part = dbias_table ? (double *)workspace : nullptr;
  hipLaunchKernelGGL(winattn_bwd_kernel, dim3(grid), dim3(NT), 0, st, qkv, bias_table, dout, dqkv, part, s);
  if (dbias_table)
    hipLaunchKernelGGL(winattn_table_kernel, dim3((unsigned)heads), dim3(NT), 0, st, (const double *)part, dbias_table,
                       heads, grid);
  return (int)hipGetLastError();
}

}  // extern "C"
