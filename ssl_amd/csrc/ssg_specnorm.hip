// Spectral normalisation of a whole set of layers in a fixed handful of launches, whatever the number of layers:
// torch.nn.utils.spectral_norm's SpectralNorm.compute_weight (dim = 0, n_power_iterations = 1, eps = 1e-12) as
// GAN-Based-SR/basicsr/archs/discriminator_arch.py (UNetDiscriminatorSN) and
// train_BSGRAN/models/network_discriminator.py (Discriminator_UNet, Discriminator_PatchGAN, Discriminator_VGG_128_SN)
// wrap their layers in it: per layer and forward two mv + normalize, two clones, a third mv, a dot and a divide, and
// autograd's walk back through them.
//
// Contract (this file is compiled with -ffp-contract=off).  W is R x K row-major fp32, u (R) and v (K) fp32.  Every
// product of two fp32 values is formed exactly in fp64, every sum is fp64 in an order fixed by INDEX (never by address
// or by arrival): the same bits from call to call, for a layer alone or among others, wherever it lies in memory.
//   training forward, three launches
//     A  tpart[b][j] = sum over the rows r of row block b (ROWS_A rows, ascending) of u_r W_rj
//     B  t_j = sum_b tpart[b][j] (ascending b);  |t|^2 = sum_j t_j t_j (thread i takes j = i, i + 256, ..., then the
//        workgroup's fold);  v_j = (float)(t_j / max(sqrt(|t|^2), eps)) stored in place and into the call's saved block;
//        s_r = sum_j W_rj v_j from that fp32 v_j (thread i takes j = i, i + 256, ..., then the workgroup's fold)
//     C  |s|^2 = sum_r s_r s_r;  u_r = (float)(s_r / max(sqrt(|s|^2), eps)) stored in place and saved;
//        sigma = sum_r u_r s_r (fp32 u_r, fp64 s_r);  sigma32 = (float)sigma saved;  out = W / sigma32, one correctly
//        rounded fp32 division per element
//   eval forward, two launches: B without t (v as stored), C with u as stored; both still fill the saved block
//   backward, two launches
//     1  bpart[c] = sum over chunk c of G (W / sigma32)  (thread i takes the groups of four i, i + 256, ... by INDEX)
//     2  c = sum of the layer's bpart (thread i takes i, i + 256, ...);
//        dW_rj = (float)((G_rj - c u_r v_j) / sigma32) in fp64 from the call's SAVED u, v, sigma32
//   max(x, eps) is `x < eps ? eps : x`: a NaN norm stays a NaN, as torch's clamp_min keeps it.  Nothing is
//   special-cased: an all-zero W gives u = v = 0 and out = 0 / 0 = NaN.  Every sum is a layer's own: a NaN stays there.
// Every quantity of the fold is recomputed by each workgroup that needs it (redundantly, in the same order): no
// atomics, no tickets, one writer per element (the workgroup of a layer's first unit stores u, v, sigma32).  LDS holds
// only the four wave sums of a fold.  No scratch.
//
// The table (8-byte words, built on the host by ssg_sn_table_fill, resident on the device, reused from call to call):
//   [0] n_layers [1] units of A [2] units of B [3] chunks [4] chunk (elements)
//   [5] floats of the output block [6] doubles of the workspace [7] floats of the saved block
//   n_layers records of eight words: W, u, v addresses, R, K, the layer's offset into the output block (floats; the
//     gradient block has the same layout), into the workspace (doubles), into the saved block (floats)
//   three prefix tables of n_layers + 1 words: the first unit of each layer in A, in B, and its first chunk
// A layer's workspace: tpart (ceil(R / ROWS_A) K doubles), s (R), bpart (its chunks).  Its saved block: u (R), v (K),
// sigma32.  A unit is found from its prefix table by bisection; grids are capped and walk grid-stride.
// This file defines the entry points ssg_sn_* at its end; they refuse bad arguments before any launch.
#include <algorithm>
#include <vector>

#include "ssg_chunked.hpp"

namespace ssg {
namespace sn {

using namespace chunked;

typedef unsigned long long word;

constexpr int STRIP = NT;         // columns of a unit of A: one per thread, a wave reads 256 consecutive bytes of a row
constexpr int ROWS_A = 64;        // rows of a unit of A: the eight UNetDiscriminatorSN layers are 269 units
constexpr int ROWS_B = 16;        // rows of a unit of B: sixteen fp64 accumulators per thread
constexpr int CHUNK = 4096;       // elements of a unit of C and of the backward: four float4 trips of a workgroup
constexpr int GRID_CAP = MAX_WG;  // the scaffold's: four workgroups per CU
constexpr double EPS = 1e-12;     // torch's default
constexpr size_t HEADER_WORDS = 8, RECORD_WORDS = 8;
enum { H_LAYERS, H_UNITS_A, H_UNITS_B, H_CHUNKS, H_CHUNK, H_OUT, H_WS, H_SAVED };
enum { L_W, L_U, L_V, L_ROWS, L_COLS, L_OUT, L_WS, L_SAVED };

SSG_TUNING tuning = {CHUNK, GRID_CAP};   // ssg_prof_sn_tuning: the A/B of profiles/specnorm_time.txt

__host__ __device__ inline size_t blocks_of(size_t n, size_t per) { return n / per + (n % per != 0); }

// one layer as a unit sees it
struct Layer {
  const float *W;
  float *u, *v;
  unsigned R, K;
  size_t out, saved;
  double *tpart, *s, *bpart;
};

struct Table {
  word n, units_a, units_b, chunks;
  unsigned chunk;
  const word *records, *first_a, *first_b, *first_c;
};

__device__ __forceinline__ Table open(const word *table) {
  Table t;
  t.n = table[H_LAYERS], t.units_a = table[H_UNITS_A], t.units_b = table[H_UNITS_B], t.chunks = table[H_CHUNKS];
  t.chunk = (unsigned)table[H_CHUNK];
  t.records = table + HEADER_WORDS;
  t.first_a = t.records + RECORD_WORDS * t.n, t.first_b = t.first_a + t.n + 1, t.first_c = t.first_b + t.n + 1;
  return t;
}

// the layer that holds `unit`: the last l with first[l] <= unit (first[0] = 0, first[n] = the unit count)
__device__ __forceinline__ unsigned layer_of(const word *first, word n, word unit) {
  unsigned lo = 0, hi = (unsigned)n;
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) / 2;
    if (first[mid] <= unit) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ Layer layer(const Table &t, unsigned l, double *ws) {
  const word *rec = t.records + RECORD_WORDS * l;
  Layer y;
  y.W = (const float *)rec[L_W], y.u = (float *)rec[L_U], y.v = (float *)rec[L_V];
  y.R = (unsigned)rec[L_ROWS], y.K = (unsigned)rec[L_COLS];
  y.out = (size_t)rec[L_OUT], y.saved = (size_t)rec[L_SAVED];
  y.tpart = ws + rec[L_WS];
  y.s = y.tpart + blocks_of(y.R, ROWS_A) * y.K;
  y.bpart = y.s + y.R;
  return y;
}

// the workgroup's NV sums, to every thread: a wave by the shuffle tree, the four waves in order, pairwise.  Every thread
// must call it; the barrier behind the reads lets the next call write again.
template <int NV>
__device__ __forceinline__ void fold_all(double (&v)[NV]) {
  __shared__ double w[NV][NT / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += __shfl_down(v[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) w[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = (w[k][0] + w[k][1]) + (w[k][2] + w[k][3]);
  __syncthreads();
}

__device__ __forceinline__ double clamped(double norm) { return norm < EPS ? EPS : norm; }   // (a NaN passes)

// ---- A: the row blocks' partial sums of t = W^T u; lanes along K ----
__global__ __launch_bounds__(NT) void sn_t_kernel(const word *table, double *ws) {
  const Table t = open(table);
  for (word unit = blockIdx.x; unit < t.units_a; unit += gridDim.x) {
    const unsigned l = layer_of(t.first_a, t.n, unit);
    const Layer y = layer(t, l, ws);
    const unsigned local = (unsigned)(unit - t.first_a[l]), strips = (unsigned)blocks_of(y.K, STRIP);
    const unsigned block = local / strips, j = (local % strips) * STRIP + threadIdx.x;
    if (j >= y.K) continue;
    const unsigned r0 = block * ROWS_A, r1 = r0 + ROWS_A < y.R ? r0 + ROWS_A : y.R;
    const float *w = y.W + (size_t)r0 * y.K + j;
    double acc = 0.0;
#pragma unroll 8
    for (unsigned r = r0; r < r1; ++r, w += y.K) acc += (double)y.u[r] * (double)*w;
    y.tpart[(size_t)block * y.K + j] = acc;
  }
}

__device__ __forceinline__ double folded_t(const Layer &y, unsigned blocks, unsigned j) {
  double t = 0.0;
  for (unsigned b = 0; b < blocks; ++b) t += y.tpart[(size_t)b * y.K + j];
  return t;
}

// ---- B: v from t (TRAIN) or as stored, and the rows' s = W v; a thread owns the columns i, i + 256, ... ----
template <bool TRAIN>
__global__ __launch_bounds__(NT) void sn_s_kernel(const word *table, double *ws, float *saved) {
  const Table t = open(table);
  for (word unit = blockIdx.x; unit < t.units_b; unit += gridDim.x) {
    const unsigned l = layer_of(t.first_b, t.n, unit);
    const Layer y = layer(t, l, ws);
    const unsigned block = (unsigned)(unit - t.first_b[l]), blocks_a = (unsigned)blocks_of(y.R, ROWS_A);
    const unsigned r0 = block * ROWS_B;
    float *saved_v = saved + y.saved + y.R;
    double den = 1.0;
    if (TRAIN) {
      double q[1] = {0.0};
      for (unsigned j = threadIdx.x; j < y.K; j += NT) {
        const double tj = folded_t(y, blocks_a, j);
        q[0] += tj * tj;
      }
      fold_all<1>(q);
      den = clamped(sqrt(q[0]));
    }
    double acc[ROWS_B];
#pragma unroll
    for (int i = 0; i < ROWS_B; ++i) acc[i] = 0.0;
    for (unsigned j = threadIdx.x; j < y.K; j += NT) {
      float vj;
      if (TRAIN) {
        vj = (float)(folded_t(y, blocks_a, j) / den);
        if (block == 0) y.v[j] = vj;
      } else {
        vj = y.v[j];
      }
      if (block == 0) saved_v[j] = vj;
      const float *w = y.W + (size_t)r0 * y.K + j;
#pragma unroll
      for (int i = 0; i < ROWS_B; ++i)
        if (r0 + i < y.R) acc[i] += (double)w[(size_t)i * y.K] * (double)vj;
    }
    fold_all<ROWS_B>(acc);
    if (threadIdx.x < ROWS_B && r0 + threadIdx.x < y.R) {
      double mine = 0.0;
#pragma unroll
      for (int i = 0; i < ROWS_B; ++i) mine = (int)threadIdx.x == i ? acc[i] : mine;
      y.s[r0 + threadIdx.x] = mine;
    }
  }
}

// ---- C: u from s (TRAIN) or as stored, sigma, and the chunk's quotients ----
template <bool TRAIN>
__global__ __launch_bounds__(NT) void sn_div_kernel(const word *table, const double *ws, float *saved, float *out) {
  const Table t = open(table);
  for (word unit = blockIdx.x; unit < t.chunks; unit += gridDim.x) {
    const unsigned l = layer_of(t.first_c, t.n, unit);
    const Layer y = layer(t, l, (double *)ws);
    const size_t ck = (size_t)(unit - t.first_c[l]);
    float *saved_u = saved + y.saved;
    double den = 1.0;
    if (TRAIN) {
      double q[1] = {0.0};
      for (unsigned r = threadIdx.x; r < y.R; r += NT) q[0] += y.s[r] * y.s[r];
      fold_all<1>(q);
      den = clamped(sqrt(q[0]));
    }
    double g[1] = {0.0};
    for (unsigned r = threadIdx.x; r < y.R; r += NT) {
      const double sr = y.s[r];
      float ur;
      if (TRAIN) {
        ur = (float)(sr / den);
        if (ck == 0) y.u[r] = ur;
      } else {
        ur = y.u[r];
      }
      if (ck == 0) saved_u[r] = ur;
      g[0] += (double)ur * sr;
    }
    fold_all<1>(g);
    const float sigma = (float)g[0];
    if (ck == 0 && threadIdx.x == 0) saved_u[(size_t)y.R + y.K] = sigma;
    const Span sp = span_of((size_t)y.R * y.K, ck, t.chunk);
    float *o = out + y.out + sp.off;
    const float *w = y.W + sp.off;
    const bool vec = wide(w, head_of(o, sp.len));
    walk_chunk(
        o, sp.len, [&](unsigned i) { o[i] = w[i] / sigma; },
        [&](unsigned i) {
          float a[4], r[4];
          load4(w + i, vec, a);
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = a[k] / sigma;
          store4(o + i, true, r);
        });
  }
}

// ---- backward 1: the chunks' partial sums of <G, W / sigma32>, groups of four by index ----
__global__ __launch_bounds__(NT) void sn_dot_kernel(const word *table, const word *grads, const float *saved, double *ws) {
  const Table t = open(table);
  for (word unit = blockIdx.x; unit < t.chunks; unit += gridDim.x) {
    const unsigned l = layer_of(t.first_c, t.n, unit);
    const float *G = (const float *)grads[l];
    if (!G) continue;                                     // (the whole workgroup: no gradient for this layer)
    const Layer y = layer(t, l, ws);
    const size_t ck = (size_t)(unit - t.first_c[l]);
    const float sigma = saved[y.saved + (size_t)y.R + y.K];
    const Span sp = span_of((size_t)y.R * y.K, ck, t.chunk);
    const float *g = G + sp.off, *w = y.W + sp.off;
    const bool vg = ((size_t)g & 15) == 0, vw = ((size_t)w & 15) == 0;
    const unsigned groups = sp.len / EPT;
    double acc[1] = {0.0};
    for (unsigned q = threadIdx.x; q < groups; q += NT) {
      float a[4], b[4];
      load4(g + EPT * q, vg, a);
      load4(w + EPT * q, vw, b);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float wsn = b[k] / sigma;
        acc[0] += (double)a[k] * (double)wsn;
      }
    }
    const unsigned e = EPT * groups + threadIdx.x;
    if (e < sp.len) {
      const float wsn = w[e] / sigma;
      acc[0] += (double)g[e] * (double)wsn;
    }
    fold_all<1>(acc);
    if (threadIdx.x == 0) y.bpart[ck] = acc[0];
  }
}

// ---- backward 2: dW = (G - <G, W_sn> u v^T) / sigma32 ----
__global__ __launch_bounds__(NT) void sn_grad_kernel(const word *table, const word *grads, const float *saved,
                                                     const double *ws, float *grad) {
  const Table t = open(table);
  for (word unit = blockIdx.x; unit < t.chunks; unit += gridDim.x) {
    const unsigned l = layer_of(t.first_c, t.n, unit);
    const float *G = (const float *)grads[l];
    if (!G) continue;
    const Layer y = layer(t, l, (double *)ws);
    const size_t ck = (size_t)(unit - t.first_c[l]);
    const unsigned chunks = (unsigned)(t.first_c[l + 1] - t.first_c[l]);
    double c[1] = {0.0};
    for (unsigned i = threadIdx.x; i < chunks; i += NT) c[0] += y.bpart[i];
    fold_all<1>(c);
    const float *su = saved + y.saved, *sv = su + y.R;
    const double sigma = (double)su[(size_t)y.R + y.K], dot = c[0];
    const Span sp = span_of((size_t)y.R * y.K, ck, t.chunk);
    float *d = grad + y.out + sp.off;
    const float *g = G + sp.off;
    const unsigned K = y.K, base = (unsigned)sp.off;
    const auto element = [&](float gi, unsigned r, unsigned j) {
      const double cu = dot * (double)su[r];
      const double cuv = cu * (double)sv[j];
      const double diff = (double)gi - cuv;
      return (float)(diff / sigma);
    };
    const bool vec = wide(g, head_of(d, sp.len));
    walk_chunk(
        d, sp.len,
        [&](unsigned i) {
          const unsigned r = (base + i) / K;
          d[i] = element(g[i], r, base + i - r * K);
        },
        [&](unsigned i) {
          float a[4], o[4];
          load4(g + i, vec, a);
          unsigned r = (base + i) / K, j = base + i - r * K;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            o[k] = element(a[k], r, j);
            if (++j == K) j = 0, ++r;
          }
          store4(d + i, true, o);
        });
  }
}

// ---- host ----
struct Counts { size_t units_a, units_b, chunks, out, ws, saved; };

constexpr size_t OUT_ALIGN = 64;   // floats: every layer's output starts on a 256-byte boundary of the block

// the set's unit counts and block sizes; false where a layer is empty, its elements or a count do not fit an int
static bool count(size_t n, const size_t *rows, const size_t *cols, size_t chunk, Counts *c) {
  Counts k = {0, 0, 0, 0, 0, 0};
  if (n > (size_t)INT_MAX) return false;
  for (size_t i = 0; i < n; ++i) {
    const size_t R = rows[i], K = cols[i];
    if (R < 1 || K < 1 || R > (size_t)INT_MAX || K > (size_t)INT_MAX || R > (size_t)INT_MAX / K) return false;
    const size_t blocks_a = blocks_of(R, ROWS_A), chunks = blocks_of(R * K, chunk);
    k.units_a += blocks_a * blocks_of(K, STRIP), k.units_b += blocks_of(R, ROWS_B), k.chunks += chunks;
    k.out += align_up(R * K, OUT_ALIGN), k.ws += blocks_a * K + R + chunks, k.saved += R + K + 1;
    if (k.units_a > (size_t)INT_MAX || k.units_b > (size_t)INT_MAX || k.chunks > (size_t)INT_MAX) return false;
  }
  *c = k;
  return true;
}

static size_t table_words(size_t n) { return HEADER_WORDS + RECORD_WORDS * n + 3 * (n + 1); }

// 0, or why a host image and the caller's blocks cannot be launched on
static int refuse(const void *table, const void *image, const void *block, size_t block_bytes, const void *workspace,
                  size_t workspace_bytes, const void *saved, size_t saved_bytes) {
  if (!table || !image || !block || !workspace || !saved) return SSG_E_BADARG;
  if (unaligned(table, sizeof(word)) || unaligned(image, sizeof(word)) || unaligned(workspace, sizeof(double)) ||
      unaligned(block, sizeof(float)) || unaligned(saved, sizeof(float)))
    return SSG_E_ALIGN;
  const word *h = (const word *)image;
  if (h[H_LAYERS] > (word)INT_MAX || h[H_UNITS_A] > (word)INT_MAX || h[H_UNITS_B] > (word)INT_MAX ||
      h[H_CHUNKS] > (word)INT_MAX)
    return SSG_E_TOOLARGE;
  if (block_bytes / sizeof(float) < h[H_OUT] || workspace_bytes / sizeof(double) < h[H_WS] ||
      saved_bytes / sizeof(float) < h[H_SAVED])
    return SSG_E_WORKSPACE;
  return 0;
}

static unsigned grid_of_units(word units) { return grid_of((size_t)units, tuning); }

}  // namespace sn
}  // namespace ssg

// ---- (Y) the entry points: every refusal is decided here, before any launch ----
using namespace ssg;

extern "C" {

int ssg_sn_chunk(void) { return sn::tuning.chunk; }

int ssg_sn_grid_cap(void) { return sn::tuning.grid_cap; }

int ssg_sn_strip(void) { return sn::STRIP; }

int ssg_sn_rows_a(void) { return sn::ROWS_A; }

int ssg_sn_rows_b(void) { return sn::ROWS_B; }

size_t ssg_sn_table_bytes(size_t n_layers, const size_t *rows, const size_t *cols) {
  sn::Counts c;
  if ((n_layers && (!rows || !cols)) || !sn::count(n_layers, rows, cols, (size_t)ssg_sn_chunk(), &c)) return 0;
  return sizeof(sn::word) * sn::table_words(n_layers);
}

size_t ssg_sn_output_bytes(size_t n_layers, const size_t *rows, const size_t *cols) {
  sn::Counts c;
  if ((n_layers && (!rows || !cols)) || !sn::count(n_layers, rows, cols, (size_t)ssg_sn_chunk(), &c)) return 0;
  return sizeof(float) * c.out;
}

size_t ssg_sn_workspace_bytes(size_t n_layers, const size_t *rows, const size_t *cols) {
  sn::Counts c;
  if ((n_layers && (!rows || !cols)) || !sn::count(n_layers, rows, cols, (size_t)ssg_sn_chunk(), &c)) return 0;
  return sizeof(double) * c.ws;
}

size_t ssg_sn_saved_bytes(size_t n_layers, const size_t *rows, const size_t *cols) {
  sn::Counts c;
  if ((n_layers && (!rows || !cols)) || !sn::count(n_layers, rows, cols, (size_t)ssg_sn_chunk(), &c)) return 0;
  return sizeof(float) * c.saved;
}

int ssg_sn_table_fill(size_t n_layers, const size_t *w, const size_t *u, const size_t *v, const size_t *rows,
                      const size_t *cols, void *table, size_t table_bytes) {
  using namespace sn;
  static_assert(sizeof(size_t) == sizeof(word), "addresses are 8-byte words");
  if (!table || (n_layers && (!w || !u || !v || !rows || !cols))) return SSG_E_BADARG;
  if (unaligned(table, sizeof(word))) return SSG_E_ALIGN;
  for (size_t i = 0; i < n_layers; ++i)
    if (rows[i] < 1 || cols[i] < 1) return SSG_E_BADARG;
  const size_t chunk = (size_t)ssg_sn_chunk();
  Counts c;
  if (!count(n_layers, rows, cols, chunk, &c)) return SSG_E_TOOLARGE;
  // every range of the set: the weights are only read, u and v are written, so no two may overlap
  std::vector<std::pair<size_t, size_t>> spans;
  spans.reserve(3 * n_layers);
  for (size_t i = 0; i < n_layers; ++i) {
    const size_t a[3] = {w[i], u[i], v[i]}, len[3] = {rows[i] * cols[i], rows[i], cols[i]};
    for (int k = 0; k < 3; ++k) {
      if (!a[k]) return SSG_E_BADARG;
      if (unaligned(a[k], sizeof(float))) return SSG_E_ALIGN;
      if (a[k] > SIZE_MAX - sizeof(float) * len[k]) return SSG_E_BADARG;     // (a range that wraps the address space)
      spans.emplace_back(a[k], a[k] + sizeof(float) * len[k]);
    }
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second) return SSG_E_BADARG;
  if (table_bytes < sizeof(word) * table_words(n_layers)) return SSG_E_WORKSPACE;
  word *out = (word *)table;
  out[H_LAYERS] = n_layers, out[H_UNITS_A] = c.units_a, out[H_UNITS_B] = c.units_b, out[H_CHUNKS] = c.chunks;
  out[H_CHUNK] = chunk, out[H_OUT] = c.out, out[H_WS] = c.ws, out[H_SAVED] = c.saved;
  word *records = out + HEADER_WORDS, *first_a = records + RECORD_WORDS * n_layers, *first_b = first_a + n_layers + 1,
       *first_c = first_b + n_layers + 1;
  Counts k = {0, 0, 0, 0, 0, 0};
  for (size_t i = 0; i < n_layers; ++i) {
    const size_t R = rows[i], K = cols[i], blocks_a = blocks_of(R, ROWS_A), chunks = blocks_of(R * K, chunk);
    word *rec = records + RECORD_WORDS * i;
    rec[L_W] = w[i], rec[L_U] = u[i], rec[L_V] = v[i], rec[L_ROWS] = R, rec[L_COLS] = K;
    rec[L_OUT] = k.out, rec[L_WS] = k.ws, rec[L_SAVED] = k.saved;
    first_a[i] = k.units_a, first_b[i] = k.units_b, first_c[i] = k.chunks;
    k.units_a += blocks_a * blocks_of(K, STRIP), k.units_b += blocks_of(R, ROWS_B), k.chunks += chunks;
    k.out += align_up(R * K, OUT_ALIGN), k.ws += blocks_a * K + R + chunks, k.saved += R + K + 1;
  }
  first_a[n_layers] = k.units_a, first_b[n_layers] = k.units_b, first_c[n_layers] = k.chunks;
  return 0;
}

int ssg_sn_forward(const void *table, const void *image, int training, float *out, size_t out_bytes, void *workspace,
                   size_t workspace_bytes, float *saved, size_t saved_bytes, ssg_stream_t stream) {
  using namespace sn;
  if (training != 0 && training != 1) return SSG_E_BADARG;
  if (const int rc = refuse(table, image, out, out_bytes, workspace, workspace_bytes, saved, saved_bytes)) return rc;
  const word *h = (const word *)image;
  if (h[H_LAYERS] == 0) return 0;                        // an empty set: nothing to launch
  const hipStream_t st = (hipStream_t)stream;
  const word *t = (const word *)table;
  double *ws = (double *)workspace;
  if (training) {
    hipLaunchKernelGGL(sn_t_kernel, dim3(grid_of_units(h[H_UNITS_A])), dim3(NT), 0, st, t, ws);
    hipLaunchKernelGGL(sn_s_kernel<true>, dim3(grid_of_units(h[H_UNITS_B])), dim3(NT), 0, st, t, ws, saved);
    hipLaunchKernelGGL(sn_div_kernel<true>, dim3(grid_of_units(h[H_CHUNKS])), dim3(NT), 0, st, t, (const double *)ws,
                       saved, out);
  } else {
    hipLaunchKernelGGL(sn_s_kernel<false>, dim3(grid_of_units(h[H_UNITS_B])), dim3(NT), 0, st, t, ws, saved);
    hipLaunchKernelGGL(sn_div_kernel<false>, dim3(grid_of_units(h[H_CHUNKS])), dim3(NT), 0, st, t, (const double *)ws,
                       saved, out);
  }
  return (int)hipGetLastError();
}

int ssg_sn_backward(const void *table, const void *image, const void *grads, const float *saved, size_t saved_bytes,
                    float *grad, size_t grad_bytes, void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  using namespace sn;
  if (!grads) return SSG_E_BADARG;
  if (unaligned(grads, sizeof(word))) return SSG_E_ALIGN;
  if (const int rc = refuse(table, image, grad, grad_bytes, workspace, workspace_bytes, saved, saved_bytes)) return rc;
  const word *h = (const word *)image;
  if (h[H_LAYERS] == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_of_units(h[H_CHUNKS]);
  hipLaunchKernelGGL(sn_dot_kernel, dim3(grid), dim3(NT), 0, st, (const word *)table, (const word *)grads, saved,
                     (double *)workspace);
  hipLaunchKernelGGL(sn_grad_kernel, dim3(grid), dim3(NT), 0, st, (const word *)table, (const word *)grads, saved,
                     (const double *)workspace, grad);
  return (int)hipGetLastError();
}

#ifdef SSG_PROFILE
// PROFILING BUILD ONLY, bound by hand in tools/specnorm_time.py and tests/test_gpu_specnorm.py (not part of
// include/ssg_hip.h): the chunk size (a multiple of 4) and grid cap that ssg_sn_chunk / ssg_sn_grid_cap, and so the
// tables filled and the launches made afterwards, use.  The product library's two are constants.
int ssg_prof_sn_tuning(int chunk, int grid_cap) {
  return sn::tuning.set(chunk, grid_cap);
}
#endif

}  // extern "C"
