// Host-side seam of the gfx950 SSG engine: every host function that one .hip file defines and another calls, declared
// once.  ssg_api.hip (the caller of nearly all of them) and every defining file include this header, so a definition
// whose signature drifts from its declaration no longer compiles instead of becoming a new overload and an undefined
// symbol when the library is loaded.  The parameter structs live in ssg_common.hpp.
// Nothing else is declared here: every other family (the data path, the criteria, the metrics, the codecs ...) defines
// its C-ABI entry points beside its kernels, and what serves them is local to that file.
#pragma once
#include "../../include/ssg_hip.h"

#include "ssg_common.hpp"

namespace ssg {

// ---- every workspace and scratch buffer of the library ----
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// lays the pieces of a buffer out one behind the other, each on a 256-byte boundary
struct Carver {
  size_t end = 0;
  size_t take(size_t bytes) { return std::exchange(end, end + align_up(bytes, 256)); }
};

// ---- the one alignment test of every entry point: an address that is no multiple of `a` (a null pointer is aligned) ----
inline bool unaligned(size_t address, size_t a) { return address % a != 0; }
inline bool unaligned(const void *p, size_t a) { return unaligned((size_t)p, a); }

// ---- ssg_fwd.hip: direct forward ----
int launch_fwd(const FwdParams &p, hipStream_t st);
const char *fwd_kernel_name(int ks, int kw);

// ---- ssg_tiny.hip: small (11,5) steps ----
bool tiny_step_supported(int ks, int kw, int C, int capacity);
int launch_tiny_step(const TinyParams &p, int C, hipStream_t st);

// ---- ssg_dense.hip: dense-tile forward ----
bool dense_supported(int ks, int kw, int C);
int dense_tile_rows(int ks);
int dense_max_tiles(int B, int H, int W, int ks);
int dense_max_strips(int B, int H, int W, int ks);
int launch_fwd_dense(const DenseParams &p, int ks, int kw, int C, hipStream_t st);
#ifdef SSG_PROFILE
int strip_times(unsigned long long *host, int n);
int strip_occupancy();
#endif

// ---- ssg_bwd.hip: direct backward, fixed-point gradient sums, loss finalize ----
int launch_bwd(const BwdParams &p, hipStream_t st);
unsigned bwd_grid(const BwdParams &p);
size_t bwd_max_partials(int B, int H, int W, int n_rows);
int launch_loss_finalize(const LossFinalize &f, hipStream_t st);
const char *bwd_kernel_name(int ks, int kw);
int launch_grad_fix_flush(long long *gfix, float *grad, size_t n, int assign, hipStream_t st,
                          const LossFinalize *fin = nullptr);
int launch_grad_fix_bound(const BwdParams &p, hipStream_t st);
int launch_grad_fix_reduce(const float *part, int n, long long *gfix, size_t n_fix, hipStream_t st);

// ---- ssg_bwd_dense.hip: dense-tile backward ----
bool dense_bwd_supported(int ks, int kw, int C);
int launch_bwd_dense(const DenseBwdParams &p, int ks, int kw, int C, hipStream_t st);

// ---- ssg_grow.hip: G rows, tile-major row pass ----
bool grow_supported(int ks, int kw);
unsigned grow_grid(int n_host);
int launch_grad_rows(const GrowParams &p, int ks, int kw, hipStream_t st);
int launch_rows_tm(const TmRowsParams &p, int ks, int kw, hipStream_t st);
int rows_tm_parts(int n_tiles);

// ---- ssg_edges.hip: edge list, rank map, forward plan ----
size_t edge_scratch_bytes(int B, int H, int W);
int launch_edge_list(const void *mask, int kind, int mask_channels, int B, int H, int W, int stride, float thr,
                     int *edges, int capacity, int *counts, int *rank, int *order, int *plan, int dense_thr,
                     int plan_tile_rows, void *scratch, void *zero_a, size_t zero_a_bytes, void *zero_b,
                     size_t zero_b_bytes, void *zero_c, size_t zero_c_bytes, hipStream_t st);
int launch_edge_mask(const float *gt, int B, int H, int W, float thr, int stride, uint8_t *out, hipStream_t st);
int launch_pos_to_mask(const int *pos, int mc, int Hp, int Wp, uint8_t *mask, hipStream_t st);
int launch_pos_relabel(const int *pos, int mc, int Hp, int Wp, int *rank, int *perm, int *dup, int *ndup, int *plan,
                       int *order2, hipStream_t st);
bool tiny_edge_list_ok(int B, int H, int W);
int launch_tiny_edge_list(const void *mask, int kind, int mask_channels, int B, int H, int W, int stride, float thr,
                          int *edges, int capacity, int *counts, int *rank, void *zero_a, size_t zero_a_bytes,
                          void *zero_b, size_t zero_b_bytes, void *zero_c, size_t zero_c_bytes, hipStream_t st);
// The forward plan, an int array of fwd_plan_bytes(): the places of its parts.  The builder's kernels write the four
// header words as plan[0..3]; host code never spells an offset out, it takes a view.
size_t fwd_plan_bytes(int B, int H, int W, int capacity);
int fwd_plan_order_offset(int B, int H, int W);
struct PlanView {
  const int *n_sparse;      // [0]: rows left to the direct kernels (the length of sparse_order)
  const int *dense_hdr;     // [1..3]: {n_heavy, tile rows, n_light} (dense_tile_count, tm_active)
  const int *tiles;         // the dense kernels' tile ids, heavy from the front, light from the back
  const int *strips;        // k_s 49: number of strips, then (strip id, first place) pairs
  const int *sparse_order;  // (capacity) tile-major order of the rows left to the direct kernels
};
__attribute__((visibility("hidden"))) PlanView plan_view(const int *plan, int B, int H, int W);   // (hidden: the library's dynamic symbols stay as they were)

// ---- ssg_api.hip ----
// host-mapped {rows for the direct kernels, dense tiles} of the device's last plan, written by the edge-list builder's
// scan kernel (nullptr: no hint wanted, or none allocated yet and `st` is being captured)
int *plan_hint_device_word(hipStream_t st);

}  // namespace ssg
