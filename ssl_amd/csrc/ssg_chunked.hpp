// What the ragged one-launch kernels over flat fp32 tensors share (ssg_multi.hip, ssg_mcrit.hip): a set of tensors is cut
// into chunks of ONE tensor each, a workgroup of 256 threads takes chunk c = blockIdx.x, then c + gridDim.x, ... under a
// grid cap, and walks its chunk with ssg_stream.hpp's walk_span: head and tail element by element, 16-byte groups
// between, any other tensor of the call through load4 / store4 with `wide`.  Every access lies inside the chunk, so
// inside [p, p + n) of its tensor.  (ssg_blindsr.hip's unit is a 2-D tile found by binary search: it is not built on this.)
#pragma once
#include <limits.h>

#include "ssg_stream.hpp"

namespace ssg {
namespace chunked {

using namespace stream;

// chunk size (elements, a multiple of 4) and grid cap of a file: constants of the product library, a mutable pair in
// the profiling build, where the file's ssg_prof_*_tuning sets them (SSG_TUNING tuning = {CHUNK, GRID_CAP};)
struct Tuning {
  int chunk, grid_cap;
  int set(int c, int cap) { return c < 4 || c % 4 || cap < 1 ? SSG_E_BADARG : (chunk = c, grid_cap = cap, 0); }
};
#ifdef SSG_PROFILE
#define SSG_TUNING static ssg::chunked::Tuning
#else
#define SSG_TUNING constexpr ssg::chunked::Tuning
#endif

// chunk k of a tensor of n elements: where it starts and how many elements it holds (for off < n: a caller that cannot
// trust k checks that first)
struct Span { size_t off; unsigned len; };

__device__ __forceinline__ Span span_of(size_t n, size_t k, unsigned chunk) {
  const size_t off = k * chunk;
  return Span{off, n - off < chunk ? (unsigned)(n - off) : chunk};
}

// the workgroup's walk over the len elements of one chunk at x: stream::walk's order, thread by thread
template <class One, class Quad>
__device__ __forceinline__ void walk_chunk(const float *x, unsigned len, One one, Quad quad) {
  walk_span<unsigned>((unsigned)head_of(x, len), len, threadIdx.x, NT, one, quad);
}

// ---- host ----
inline size_t chunks_of(size_t n, size_t chunk) { return n / chunk + (n % chunk != 0); }

// the number of chunks of a set; false where a tensor's or the set's count does not fit an int (SSG_E_TOOLARGE)
inline bool count_chunks(size_t n_tensors, const size_t *counts, size_t chunk, size_t *total) {
  size_t sum = 0;
  for (size_t i = 0; i < n_tensors; ++i) {
    const size_t c = chunks_of(counts[i], chunk);
    if (c > (size_t)INT_MAX || sum + c > (size_t)INT_MAX) return false;
    sum += c;
  }
  *total = sum;
  return true;
}

// one workgroup per chunk, at most the cap
inline unsigned grid_of(size_t n_chunks, const Tuning &t) {
  return (unsigned)(n_chunks < (size_t)t.grid_cap ? n_chunks : (size_t)t.grid_cap);
}

}  // namespace chunked
}  // namespace ssg
