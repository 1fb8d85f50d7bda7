// The EMA and copy updates of a whole parameter set as ONE launch, whatever the number of tensors:
// GAN-Based-SR/basicsr/models/base_model.py:75-82 (model_ema) and train_BSGRAN/models/model_base.py:192-197 (update_E),
// `ema[k].data.mul_(decay).add_(net[k].data, alpha=1 - decay)` in a Python loop over the parameter names, and
// Diffusion-Based-SR/ldm/modules/ema.py (LitEma: forward, copy_to, store, restore), `shadow.sub_(w * (shadow - param))`.
// For RRDBNet these loops are 1,404 and about 2,100 device operations per iteration, most of them on 32 or 64 elements.
//
// Contract (this file is compiled with -ffp-contract=off; the one fused operation is written out).  Per element, fp32:
//   SSG_MT_EMA   e <- fmaf(a, p, fl(e * d))            torch's e.mul_(d).add_(p, alpha=a), bit for bit
//   SSG_MT_LIT   e <- e - fl(w * fl(e - p))            three roundings, no fma; w = w_dev[0], read ON THE DEVICE
//   SSG_MT_COPY  e <- p                                a 32-bit move: every bit pattern, NaN payloads included, passes
// Nothing is special-cased: d = 0 with an infinite e gives NaN, as the reference's product does.
//
// The table (8-byte words, built on the host by ssg_multi_table_fill, resident on the device, reused from call to call):
//   [0] n_tensors  [1] n_chunks  [2] chunk (elements)  [3] 0
//   n_tensors records of three words   dst address, src address, n (elements)
//   n_chunks words                     tensor index << 32 | index of the chunk inside that tensor
// in tensor order and, inside a tensor, in chunk order; an empty tensor has a record and no chunk.  Chunks, their
// schedule (at most ssg_multi_grid_cap() workgroups) and their walk are ssg_chunked.hpp's: the walked tensor is dst,
// always accessed 16 bytes wide between its head and tail; src is read 16 bytes wide where it shares dst's alignment
// and element by element where it does not.  A chunk word that points outside the table's own tensors or past a
// tensor's end is skipped.  No LDS, no atomics, no scratch.
// This file defines the entry points ssg_multi_* at its end; ssg_multi_apply refuses bad arguments before the launch.
//
// The Adam / AdamW step of a whole parameter group as ONE launch (namespace adam below, entry points ssg_adam_*):
// torch.optim.Adam / AdamW as GAN-Based-SR/basicsr/models/base_model.py:103-120 (get_optimizer),
// train_BSGRAN/models/model_ssl.py:229-230 and the Diffusion fork's configure_optimizers build them; with torch's defaults
// a chain of _foreach_ passes over the set.  Contract per element, fp32, every operation rounded on its own, `/` and sqrtf
// correctly rounded (the scalars are ssg_adam_scalars, formed on the host in double and cast once):
//   g' = g                               SSG_ADAM_PLAIN
//   g' = fl(g + fl(wd p))                SSG_ADAM_L2         (Adam's weight decay)
//   p' = fl(p cwd)                       SSG_ADAM_DECOUPLED  (AdamW's; p' = p otherwise)
//   m  <- fl(m + fl(w1 fl(g' - m)))
//   v  <- fl(fl(v b2) + fl(w2 fl(g' g')))
//   den = fl(fl(sqrtf(v) / s2) + eps)
//   p  <- fl(p' - fl(a fl(m / den)))
// Nothing is special-cased: NaN and infinite gradients propagate as the formulas say.
// The table (8-byte words, built on the host by ssg_adam_table_fill): the header above, n_tensors records of four words
// (p address, m address, v address, n), the chunk words; and BESIDE it an array of n_tensors words, the g addresses:
// gradients move between steps under zero_grad(set_to_none=True), and a moved gradient then costs an upload of that
// array (ssg_adam_grads_fill), not a rebuild of the chunk list.  The walked tensor is p; g, m and v are accessed 16 bytes
// wide where all three share p's alignment and element by element otherwise (one decision per chunk).
#include <algorithm>
#include <vector>

#include "ssg_chunked.hpp"

namespace ssg {
namespace multi {

using namespace chunked;

typedef unsigned long long word;

constexpr int CHUNK = 4096;       // elements per chunk: four float4 trips of a workgroup (profiles/ema_time.txt)
constexpr int GRID_CAP = MAX_WG;  // the scaffold's: four workgroups per CU
constexpr size_t HEADER_WORDS = 4, RECORD_WORDS = 3;

SSG_TUNING tuning = {CHUNK, GRID_CAP};   // ssg_prof_multi_tuning: the A/B of profiles/ema_time.txt

template <int KIND>
__device__ __forceinline__ float updated(float e, float p, float d, float a) {
  if (KIND == SSG_MT_EMA) return fmaf(a, p, e * d);
  if (KIND == SSG_MT_LIT) {
    const float diff = e - p;
    const float step = a * diff;   // (a holds w for this kind)
    return e - step;
  }
  return p;
}

template <int KIND>
__global__ __launch_bounds__(NT) void multi_kernel(const word *table, float d, float a, const float *w) {
  const word n_tensors = table[0], n_chunks = table[1];
  const unsigned chunk = (unsigned)table[2];
  const word *records = table + HEADER_WORDS, *chunks = records + RECORD_WORDS * n_tensors;
  if (KIND == SSG_MT_LIT) a = w[0];
  for (word c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const word cw = chunks[c], ti = cw >> 32;
    if (ti >= n_tensors) continue;
    const word *rec = records + RECORD_WORDS * ti;
    const Span sp = span_of((size_t)rec[2], (size_t)(cw & 0xffffffffull), chunk);
    if (sp.off >= (size_t)rec[2]) continue;
    float *e = (float *)rec[0] + sp.off;
    const float *p = (const float *)rec[1] + sp.off;
    // (the chunk's one decision is taken in front of the walk: with `wide` inside the group function the compiler
    // merges load4's two forms into a 12-byte and a 4-byte load for both, which costs the aligned set 3 %)
    const auto walk_with = [&](auto pv) {
      walk_chunk(
          e, sp.len, [&](unsigned i) { e[i] = updated<KIND>(KIND == SSG_MT_COPY ? 0.f : e[i], p[i], d, a); },
          [&](unsigned i) {
            float ve[4] = {0.f, 0.f, 0.f, 0.f}, vp[4], r[4];
            if (KIND != SSG_MT_COPY) load4(e + i, true, ve);
            load4(p + i, decltype(pv)::value, vp);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = updated<KIND>(ve[k], vp[k], d, a);
            store4(e + i, true, r);
          });
    };
    if (wide(p, head_of(e, sp.len))) walk_with(std::true_type{});
    else walk_with(std::false_type{});
  }
}

static size_t table_words(size_t n_tensors, size_t n_chunks) { return HEADER_WORDS + RECORD_WORDS * n_tensors + n_chunks; }

}  // namespace multi

namespace adam {

using namespace chunked;
using multi::word;
using multi::HEADER_WORDS;

using multi::tuning;              // one chunk size and grid cap for the file: ssg_multi_chunk(), ssg_multi_grid_cap()

constexpr size_t RECORD_WORDS = 4;

// one element; -ffp-contract=off keeps every line one rounding
template <int MODE>
__device__ __forceinline__ void element(float &p, float g, float &m, float &v, const ssg_adam_scalars &s) {
  float q = p;
  if (MODE == SSG_ADAM_L2) {
    const float decay = s.wd * p;
    g = g + decay;
  }
  if (MODE == SSG_ADAM_DECOUPLED) q = p * s.cwd;
  const float diff = g - m;
  const float lerp = s.w1 * diff;
  m = m + lerp;
  const float kept = v * s.b2;
  const float sq = g * g;
  const float added = s.w2 * sq;
  v = kept + added;
  const float root = sqrtf(v);
  const float scaled = root / s.s2;
  const float den = scaled + s.eps;
  const float ratio = m / den;
  const float step = s.a * ratio;
  p = q - step;
}

template <int MODE>
__global__ __launch_bounds__(NT) void adam_kernel(const word *table, const word *grads, ssg_adam_scalars s) {
  const word n_tensors = table[0], n_chunks = table[1];
  const unsigned chunk = (unsigned)table[2];
  const word *records = table + HEADER_WORDS, *chunks = records + RECORD_WORDS * n_tensors;
  for (word c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const word cw = chunks[c], ti = cw >> 32;
    if (ti >= n_tensors) continue;
    const word *rec = records + RECORD_WORDS * ti;
    const Span sp = span_of((size_t)rec[3], (size_t)(cw & 0xffffffffull), chunk);
    if (sp.off >= (size_t)rec[3]) continue;
    float *p = (float *)rec[0] + sp.off, *m = (float *)rec[1] + sp.off, *v = (float *)rec[2] + sp.off;
    const float *g = (const float *)grads[ti] + sp.off;
    // (the chunk's one decision in front of the walk, as in multi_kernel)
    const auto walk_with = [&](auto w) {
      walk_chunk(
          p, sp.len,
          [&](unsigned i) {
            float pi = p[i], mi = m[i], vi = v[i];
            element<MODE>(pi, g[i], mi, vi, s);
            p[i] = pi, m[i] = mi, v[i] = vi;
          },
          [&](unsigned i) {
            float vp[4], vg[4], vm[4], vv[4];
            load4(p + i, true, vp);
            load4(g + i, decltype(w)::value, vg);
            load4(m + i, decltype(w)::value, vm);
            load4(v + i, decltype(w)::value, vv);
#pragma unroll
            for (int k = 0; k < 4; ++k) element<MODE>(vp[k], vg[k], vm[k], vv[k], s);
            store4(p + i, true, vp);
            store4(m + i, decltype(w)::value, vm);
            store4(v + i, decltype(w)::value, vv);
          });
    };
    const size_t head = head_of(p, sp.len);
    if (wide(g, head) && wide(m, head) && wide(v, head)) walk_with(std::true_type{});
    else walk_with(std::false_type{});
  }
}

static size_t table_words(size_t n_tensors, size_t n_chunks) { return HEADER_WORDS + RECORD_WORDS * n_tensors + n_chunks; }

// 0, or why these addresses cannot be stepped: a null or misaligned address of a non-empty tensor, or two of the 4 n
// ranges that overlap (p, m, v: arrays, or the records of a filled image with stride RECORD_WORDS)
static int refuse(size_t n_tensors, const word *p, const word *m, const word *v, size_t stride, const size_t *g,
                  const word *counts) {
  std::vector<std::pair<size_t, size_t>> spans;
  spans.reserve(4 * n_tensors);
  for (size_t i = 0; i < n_tensors; ++i) {
    const size_t n = (size_t)counts[stride * i];
    if (n == 0) continue;                               // (an empty tensor's pointers are never used)
    const size_t a[4] = {(size_t)p[stride * i], (size_t)m[stride * i], (size_t)v[stride * i], g[i]};
    for (size_t x : a) {
      if (!x) return SSG_E_BADARG;
      if (unaligned(x, sizeof(float))) return SSG_E_ALIGN;
      spans.emplace_back(x, x + sizeof(float) * n);
    }
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second) return SSG_E_BADARG;
  return 0;
}

}  // namespace adam

}  // namespace ssg

// ---- (S) the entry points: every refusal is decided here, before the launch ----
using namespace ssg;

extern "C" {

int ssg_multi_chunk(void) { return multi::tuning.chunk; }

int ssg_multi_grid_cap(void) { return multi::tuning.grid_cap; }

size_t ssg_multi_chunks(size_t n_tensors, const size_t *counts) {
  size_t total = 0;
  if (n_tensors && !counts) return 0;
  return multi::count_chunks(n_tensors, counts, (size_t)ssg_multi_chunk(), &total) ? total : (size_t)INT_MAX + 1;
}

size_t ssg_multi_table_bytes(size_t n_tensors, const size_t *counts) {
  size_t total = 0;
  if ((n_tensors && !counts) || n_tensors > (size_t)INT_MAX) return 0;
  if (!multi::count_chunks(n_tensors, counts, (size_t)ssg_multi_chunk(), &total)) return 0;
  return sizeof(multi::word) * multi::table_words(n_tensors, total);
}

int ssg_multi_table_fill(size_t n_tensors, const size_t *dst, const size_t *src, const size_t *counts, void *table,
                         size_t table_bytes) {
  using namespace multi;
  if (!table || (n_tensors && (!dst || !src || !counts))) return SSG_E_BADARG;
  if (unaligned(table, sizeof(word))) return SSG_E_ALIGN;
  if (n_tensors > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  const size_t chunk = (size_t)ssg_multi_chunk();
  size_t total = 0;
  if (!count_chunks(n_tensors, counts, chunk, &total)) return SSG_E_TOOLARGE;
  for (size_t i = 0; i < n_tensors; ++i) {
    if (counts[i] == 0) continue;                     // (an empty tensor's pointers are never used)
    if (!dst[i] || !src[i]) return SSG_E_BADARG;
    if (unaligned(dst[i], sizeof(float)) || unaligned(src[i], sizeof(float))) return SSG_E_ALIGN;
  }
  if (table_bytes < sizeof(word) * table_words(n_tensors, total)) return SSG_E_WORKSPACE;
  word *out = (word *)table;
  out[0] = n_tensors, out[1] = total, out[2] = chunk, out[3] = 0;
  word *records = out + HEADER_WORDS, *chunks = records + RECORD_WORDS * n_tensors;
  for (size_t i = 0; i < n_tensors; ++i) {
    records[RECORD_WORDS * i] = dst[i], records[RECORD_WORDS * i + 1] = src[i], records[RECORD_WORDS * i + 2] = counts[i];
    for (size_t k = 0; k * chunk < counts[i]; ++k) *chunks++ = (word)i << 32 | k;
  }
  return 0;
}

int ssg_multi_apply(const void *table, size_t n_chunks, int kind, float d, float a, const float *w_dev,
                    ssg_stream_t stream) {
  if (!table || kind < SSG_MT_EMA || kind > SSG_MT_COPY || d != d || a != a) return SSG_E_BADARG;
  if (kind == SSG_MT_LIT && !w_dev) return SSG_E_BADARG;
  if (unaligned(table, sizeof(multi::word)) || unaligned(w_dev, sizeof(float))) return SSG_E_ALIGN;
  if (n_chunks > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  if (n_chunks == 0) return 0;                          // a set of empty tensors: nothing to launch
  using namespace multi;
  const auto go = [&](auto k) {
    hipLaunchKernelGGL(multi_kernel<decltype(k)::value>, dim3(grid_of(n_chunks, tuning)), dim3(NT), 0, (hipStream_t)stream,
                       (const word *)table, d, a, w_dev);
  };
  if (kind == SSG_MT_EMA) go(std::integral_constant<int, SSG_MT_EMA>{});
  else if (kind == SSG_MT_LIT) go(std::integral_constant<int, SSG_MT_LIT>{});
  else go(std::integral_constant<int, SSG_MT_COPY>{});
  return (int)hipGetLastError();
}

// ---- the Adam / AdamW step ----
size_t ssg_adam_table_bytes(size_t n_tensors, const size_t *counts) {
  size_t total = 0;
  if ((n_tensors && !counts) || n_tensors > (size_t)INT_MAX) return 0;
  if (!adam::count_chunks(n_tensors, counts, (size_t)ssg_multi_chunk(), &total)) return 0;
  return sizeof(adam::word) * adam::table_words(n_tensors, total);
}

int ssg_adam_table_fill(size_t n_tensors, const size_t *p, const size_t *g, const size_t *m, const size_t *v,
                        const size_t *counts, void *table, size_t table_bytes, void *grads, size_t grads_bytes) {
  using namespace adam;
  static_assert(sizeof(size_t) == sizeof(word), "addresses are 8-byte words");
  if (!table || !grads || (n_tensors && (!p || !g || !m || !v || !counts))) return SSG_E_BADARG;
  if (unaligned(table, sizeof(word)) || unaligned(grads, sizeof(word))) return SSG_E_ALIGN;
  if (n_tensors > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  const size_t chunk = (size_t)ssg_multi_chunk();
  size_t total = 0;
  if (!count_chunks(n_tensors, counts, chunk, &total)) return SSG_E_TOOLARGE;
  if (const int rc = refuse(n_tensors, (const word *)p, (const word *)m, (const word *)v, 1, g, (const word *)counts))
    return rc;
  if (table_bytes < sizeof(word) * table_words(n_tensors, total) || grads_bytes < sizeof(word) * n_tensors)
    return SSG_E_WORKSPACE;
  word *out = (word *)table, *gout = (word *)grads;
  out[0] = n_tensors, out[1] = total, out[2] = chunk, out[3] = 0;
  word *records = out + HEADER_WORDS, *chunks = records + RECORD_WORDS * n_tensors;
  for (size_t i = 0; i < n_tensors; ++i) {
    word *rec = records + RECORD_WORDS * i;
    rec[0] = p[i], rec[1] = m[i], rec[2] = v[i], rec[3] = counts[i], gout[i] = g[i];
    for (size_t k = 0; k * chunk < counts[i]; ++k) *chunks++ = (word)i << 32 | k;
  }
  return 0;
}

int ssg_adam_grads_fill(const void *table, size_t n_tensors, const size_t *g, void *grads, size_t grads_bytes) {
  using namespace adam;
  if (!table || !grads || (n_tensors && !g)) return SSG_E_BADARG;
  if (unaligned(table, sizeof(word)) || unaligned(grads, sizeof(word))) return SSG_E_ALIGN;
  const word *in = (const word *)table, *records = in + HEADER_WORDS;
  if (in[0] != n_tensors) return SSG_E_BADARG;          // (the image of another set)
  if (const int rc = refuse(n_tensors, records, records + 1, records + 2, RECORD_WORDS, g, records + 3)) return rc;
  if (grads_bytes < sizeof(word) * n_tensors) return SSG_E_WORKSPACE;
  for (size_t i = 0; i < n_tensors; ++i) ((word *)grads)[i] = g[i];
  return 0;
}

int ssg_adam_apply(const void *table, const void *grads, size_t n_chunks, const ssg_adam_scalars *scalars,
                   ssg_stream_t stream) {
  if (!table || !grads || !scalars) return SSG_E_BADARG;
  if (scalars->mode < SSG_ADAM_PLAIN || scalars->mode > SSG_ADAM_DECOUPLED) return SSG_E_BADARG;
  if (unaligned(table, sizeof(adam::word)) || unaligned(grads, sizeof(adam::word)) || unaligned(scalars, sizeof(float)))
    return SSG_E_ALIGN;
  if (n_chunks > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  if (n_chunks == 0) return 0;                          // a set of empty tensors: nothing to launch
  using namespace adam;
  const auto go = [&](auto k) {
    hipLaunchKernelGGL(adam_kernel<decltype(k)::value>, dim3(grid_of(n_chunks, tuning)), dim3(NT), 0, (hipStream_t)stream,
                       (const word *)table, (const word *)grads, *scalars);
  };
  if (scalars->mode == SSG_ADAM_PLAIN) go(std::integral_constant<int, SSG_ADAM_PLAIN>{});
  else if (scalars->mode == SSG_ADAM_L2) go(std::integral_constant<int, SSG_ADAM_L2>{});
  else go(std::integral_constant<int, SSG_ADAM_DECOUPLED>{});
  return (int)hipGetLastError();
}

#ifdef SSG_PROFILE
// PROFILING BUILD ONLY, bound by hand in tools/ema_time.py (not part of include/ssg_hip.h): the chunk size (a multiple of
// 4) and grid cap that ssg_multi_chunk / ssg_multi_grid_cap, and so the tables filled and the launches made afterwards,
// use: the A/B of profiles/ema_time.txt.  The product library's two are constants.
int ssg_prof_multi_tuning(int chunk, int grid_cap) {
  return multi::tuning.set(chunk, grid_cap);
}
#endif

}  // extern "C"
