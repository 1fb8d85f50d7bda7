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
// in tensor order and, inside a tensor, in chunk order; an empty tensor has a record and no chunk.  A workgroup of 256
// threads takes chunk c = blockIdx.x, then c + gridDim.x, ... (at most ssg_multi_grid_cap() workgroups).  The chunk
// covers elements [k chunk, min(n, (k + 1) chunk)) of its tensor; it is walked as ssg_stream.hpp walks a tensor: the
// elements in front of dst's first 16-byte boundary and behind the last whole float4 one by one, the rest 16 bytes wide
// where src shares dst's alignment, element by element where it does not.  Every store lies inside the chunk, so inside
// [dst, dst + n) of its tensor.  A chunk word that points outside the table's own tensors or past a tensor's end is
// skipped.  No LDS, no atomics, no scratch.
// The launcher trusts its arguments: ssg_multi_apply below refuses bad ones before the launch.
#include <limits.h>

#include <type_traits>

#include "ssg_stream.hpp"

namespace ssg {
namespace multi {

using namespace stream;

typedef unsigned long long word;

constexpr int CHUNK = 4096;       // elements per chunk: four float4 trips of a workgroup (profiles/ema_time.txt)
constexpr int GRID_CAP = MAX_WG;  // the scaffold's: four workgroups per CU
constexpr size_t HEADER_WORDS = 4, RECORD_WORDS = 3;

#ifdef SSG_PROFILE
static int g_chunk = CHUNK, g_grid_cap = GRID_CAP;   // ssg_prof_multi_tuning: the A/B of profiles/ema_time.txt
#else
constexpr int g_chunk = CHUNK, g_grid_cap = GRID_CAP;
#endif

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
  const unsigned t = threadIdx.x;
  for (word c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const word cw = chunks[c], ti = cw >> 32;
    if (ti >= n_tensors) continue;
    const word *rec = records + RECORD_WORDS * ti;
    const size_t n = (size_t)rec[2], off = (size_t)(cw & 0xffffffffull) * chunk;
    if (off >= n) continue;
    const unsigned len = n - off < chunk ? (unsigned)(n - off) : chunk;
    float *e = (float *)rec[0] + off;
    const float *p = (const float *)rec[1] + off;
    const auto one = [&](unsigned i) { e[i] = updated<KIND>(KIND == SSG_MT_COPY ? 0.f : e[i], p[i], d, a); };
    const unsigned head = (unsigned)head_of(e, len);
    if (wide(p, head)) {
      const unsigned n4 = (len - head) / EPT, tail = head + EPT * n4;
      if (t < head) one(t);
      for (unsigned q = t; q < n4; q += NT) {
        float ve[4] = {0.f, 0.f, 0.f, 0.f}, vp[4], r[4];
        if (KIND != SSG_MT_COPY) load4(e + head + EPT * q, true, ve);
        load4(p + head + EPT * q, true, vp);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = updated<KIND>(ve[k], vp[k], d, a);
        store4(e + head + EPT * q, true, r);
      }
      if (tail + t < len) one(tail + t);
    } else {
      for (unsigned i = t; i < len; i += NT) one(i);
    }
  }
}

// the number of chunks of a set; false where a tensor's or the set's count does not fit (SSG_E_TOOLARGE)
static bool count_chunks(size_t n_tensors, const size_t *counts, size_t chunk, size_t *total) {
  size_t sum = 0;
  for (size_t i = 0; i < n_tensors; ++i) {
    const size_t c = counts[i] / chunk + (counts[i] % chunk != 0);
    if (c > (size_t)INT_MAX || sum + c > (size_t)INT_MAX) return false;
    sum += c;
  }
  *total = sum;
  return true;
}

static size_t table_words(size_t n_tensors, size_t n_chunks) { return HEADER_WORDS + RECORD_WORDS * n_tensors + n_chunks; }

}  // namespace multi

int multi_chunk() { return multi::g_chunk; }

int multi_grid_cap() { return multi::g_grid_cap; }

int launch_multi_apply(const void *table, size_t n_chunks, int kind, float d, float a, const float *w, hipStream_t st) {
  using namespace multi;
  const unsigned grid = (unsigned)(n_chunks < (size_t)g_grid_cap ? n_chunks : (size_t)g_grid_cap);
  const auto go = [&](auto k) {
    hipLaunchKernelGGL(multi_kernel<decltype(k)::value>, dim3(grid), dim3(NT), 0, st, (const word *)table, d, a, w);
  };
  if (kind == SSG_MT_EMA) go(std::integral_constant<int, SSG_MT_EMA>{});
  else if (kind == SSG_MT_LIT) go(std::integral_constant<int, SSG_MT_LIT>{});
  else go(std::integral_constant<int, SSG_MT_COPY>{});
  return (int)hipGetLastError();
}

}  // namespace ssg

// ---- (S) the entry points: every refusal is decided here, before the launch ----
using namespace ssg;

extern "C" {

int ssg_multi_chunk(void) { return multi_chunk(); }

int ssg_multi_grid_cap(void) { return multi_grid_cap(); }

size_t ssg_multi_chunks(size_t n_tensors, const size_t *counts) {
  size_t total = 0;
  if (n_tensors && !counts) return 0;
  return multi::count_chunks(n_tensors, counts, (size_t)multi_chunk(), &total) ? total : (size_t)INT_MAX + 1;
}

size_t ssg_multi_table_bytes(size_t n_tensors, const size_t *counts) {
  size_t total = 0;
  if ((n_tensors && !counts) || n_tensors > (size_t)INT_MAX) return 0;
  if (!multi::count_chunks(n_tensors, counts, (size_t)multi_chunk(), &total)) return 0;
  return sizeof(multi::word) * multi::table_words(n_tensors, total);
}

int ssg_multi_table_fill(size_t n_tensors, const size_t *dst, const size_t *src, const size_t *counts, void *table,
                         size_t table_bytes) {
  using namespace multi;
  if (!table || (n_tensors && (!dst || !src || !counts))) return SSG_E_BADARG;
  if ((size_t)table % sizeof(word)) return SSG_E_ALIGN;
  if (n_tensors > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  const size_t chunk = (size_t)multi_chunk();
  size_t total = 0;
  if (!count_chunks(n_tensors, counts, chunk, &total)) return SSG_E_TOOLARGE;
  for (size_t i = 0; i < n_tensors; ++i) {
    if (counts[i] == 0) continue;                     // (an empty tensor's pointers are never used)
    if (!dst[i] || !src[i]) return SSG_E_BADARG;
    if (dst[i] % sizeof(float) || src[i] % sizeof(float)) return SSG_E_ALIGN;
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
  if ((size_t)table % sizeof(multi::word) || (size_t)w_dev % sizeof(float)) return SSG_E_ALIGN;
  if (n_chunks > (size_t)INT_MAX) return SSG_E_TOOLARGE;
  if (n_chunks == 0) return 0;                          // a set of empty tensors: nothing to launch
  return launch_multi_apply(table, n_chunks, kind, d, a, w_dev, (hipStream_t)stream);
}

#ifdef SSG_PROFILE
// PROFILING BUILD ONLY, bound by hand in tools/ema_time.py (not part of include/ssg_hip.h): the chunk size (a multiple of
// 4) and grid cap that ssg_multi_chunk / ssg_multi_grid_cap, and so the tables filled and the launches made afterwards,
// use: the A/B of profiles/ema_time.txt.  The product library's two are constants.
int ssg_prof_multi_tuning(int chunk, int grid_cap) {
  if (chunk < 4 || chunk % 4 || grid_cap < 1) return SSG_E_BADARG;
  multi::g_chunk = chunk, multi::g_grid_cap = grid_cap;
  return 0;
}
#endif

}  // extern "C"
