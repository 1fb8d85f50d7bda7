// Host-side seam of the gfx950 SSG engine: every host function that one .hip file defines and another calls, declared
// once.  ssg_api.hip (the caller of nearly all of them) and every defining file include this header, so a definition
// whose signature drifts from its declaration no longer compiles instead of becoming a new overload and an undefined
// symbol when the library is loaded.  The parameter structs live in ssg_common.hpp.
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

// ---- ssg_grow.hip: G rows, tile-major row pass, criteria on foreign tensors ----
bool grow_supported(int ks, int kw);
unsigned grow_grid(int n_host);
int launch_grad_rows(const GrowParams &p, int ks, int kw, hipStream_t st);
int launch_rows_tm(const TmRowsParams &p, int ks, int kw, hipStream_t st);
int rows_tm_parts(int n_tiles);
size_t criteria_scratch_bytes();
int launch_criteria_sums(const float *a, const float *b, size_t n, void *scratch, float *sums_out, hipStream_t st);
int launch_criteria_grad(const float *a, const float *b, size_t n, const float *coef, float *g, hipStream_t st);

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
int fwd_plan_strip_offset(int B, int H, int W);
int fwd_plan_order_offset(int B, int H, int W);
struct PlanView {
  const int *n_sparse;      // [0]: rows left to the direct kernels (the length of sparse_order)
  const int *dense_hdr;     // [1..3]: {n_heavy, tile rows, n_light} (dense_tile_count, tm_active)
  const int *tiles;         // the dense kernels' tile ids, heavy from the front, light from the back
  const int *strips;        // k_s 49: number of strips, then (strip id, first place) pairs
  const int *sparse_order;  // (capacity) tile-major order of the rows left to the direct kernels
};
__attribute__((visibility("hidden"))) PlanView plan_view(const int *plan, int B, int H, int W);   // (hidden: the library's dynamic symbols stay as they were)

// ---- ssg_datapath.hip: crop, pool swap, USM sharpening, filter2d, DiffJPEG ----
int launch_augment_crop(const void *src, void *dst, int elem_bytes, int B, int C, int Hs, int Ws, int Ho, int Wo,
                        const int *params, hipStream_t st);
int launch_pool_swap(void *queue, void *batch, size_t sample_bytes, const int *slots, int b, hipStream_t st);
size_t usm_scratch_bytes(int B, int C, int H, int W);
int launch_usm_sharp(const float *img, float *out, int B, int C, int H, int W, int ksize, float sigma, float weight,
                     float threshold, void *scratch, hipStream_t st);
int launch_filter2d(const float *img, const float *kernels, float *out, int B, int C, int H, int W, int k, int nk,
                    hipStream_t st);
int launch_jpeg(const float *img, float *out, int B, int H, int W, const float *quality_dev, float quality_host,
                hipStream_t st);

// ---- ssg_kernels.hip: the degradation chain's blur / sinc / pulse kernels from their parameter records ----
constexpr int SYNTH_MAX_PAD = 21;   // the largest padded kernel (stock Real-ESRGAN's; filter2d's largest k)
int launch_synth_kernels(const ssg_kernel_record *records_dev, int n, int pad_to, float *out, hipStream_t st);

// ---- ssg_metrics.hip: PSNR / SSIM (its entry points are defined beside its kernels) ----
size_t metric_workspace_bytes(int B, int C, int H, int W, int crop);

// ---- ssg_niqe.hip: NIQE (entry points beside its kernels; nothing of it is called from another file) ----

// ---- ssg_colorfix.hip: wavelet / AdaIN colour correction (entry points beside its kernels; nothing of it is called
// from another file) ----

// ---- ssg_ssim.hip: KAIR's SSIM criterion, loss and gradient in two launches ----
int ssim_grid_cap();
int ssim_taps(int window_size, float *taps);                  // host only: the 11 centred fp32 taps
size_t ssim_workspace_bytes(int B, int C, int H, int W);
int launch_ssim_loss(const float *x, const float *y, int B, int C, int H, int W, int window_size, float *grad_x,
                     double *sums_out, void *workspace, size_t workspace_bytes, hipStream_t st);

// ---- ssg_gan.hip: the GAN criteria, plain and relativistic: sum l and sum l' in one pass, the gradient in one ----
int gan_grid_cap();
size_t gan_workspace_bytes();
int launch_gan_sums(const float *x, size_t n, int kind, float sign, float label, const float *shift, void *workspace,
                    double *sums_out, hipStream_t st);
int launch_gan_grad(const float *x, size_t n, int kind, float sign, float label, const float *shift, const double *coef,
                    float *grad, hipStream_t st);

// ---- ssg_spsr.hip: SPSR's gradient map, its adjoint, the criteria fused on it, the streaming pixel criteria ----
int spsr_grid_cap();
size_t spsr_workspace_bytes();
int launch_spsr_map(const float *x, int planes, int H, int W, float *map, hipStream_t st);
int launch_spsr_loss(const float *x, const float *t, int planes, int H, int W, int kind, float eps, float *map_out,
                     void *workspace, double *sum_out, hipStream_t st);
// t == nullptr: the map's own adjoint of gmap; else the fused loss's, coef[0] crit' (+ gmap where given)
int launch_spsr_gather(const float *x, const float *t, const float *gmap, const double *coef, int planes, int H, int W,
                       int kind, float eps, float *dx, hipStream_t st);
int launch_spsr_branch_sums(const float *branch, const float *gt, int planes, int H, int W, int kind, float eps,
                            void *workspace, double *sum_out, hipStream_t st);
int launch_spsr_branch_grad(const float *branch, const float *gt, int planes, int H, int W, int kind, float eps,
                            const double *coef, float *grad, hipStream_t st);
int launch_pixel_sums(const float *a, const float *b, size_t n, int kind, float eps, void *workspace, double *sum_out,
                      hipStream_t st);
int launch_pixel_grad(const float *a, const float *b, size_t n, int kind, float eps, const double *coef, float *grad,
                      hipStream_t st);

// ---- ssg_multi.hip: the EMA / copy update of a whole parameter set in one launch (entry points beside its kernel) ----
int multi_chunk();
int multi_grid_cap();
int launch_multi_apply(const void *table, size_t n_chunks, int kind, float d, float a, const float *w, hipStream_t st);

// ---- ssg_mcrit.hip: a pixel criterion over a ragged set of tensor pairs, one launch each way (entry points beside its
// kernels) ----
int mcrit_chunk();
int mcrit_grid_cap();
int launch_mcrit_sums(size_t K, const size_t *x, const size_t *g, const size_t *counts, const double *w, int kind,
                      float eps, void *workspace, double *sums_out, hipStream_t st);
int launch_mcrit_grad(size_t K, const size_t *x, const size_t *g, const size_t *grad, const size_t *counts,
                      const double *w, int kind, float eps, const double *sums, const double *coef, hipStream_t st);

// ---- ssg_diffusion.hip: the Diffusion fork's schedule combinations, p_sample, training criterion and canvas stitch ----
int diff_chunk();
int diff_grid_cap();
bool diff_chunks(size_t B, size_t n, size_t *per_sample, size_t *total);
int launch_diff_combine(const float *x, const float *y, const long long *t, const float *A, const float *Bt, int T,
                        size_t B, size_t n, int subtract, int clamp, float lo, float hi, float *out, hipStream_t st);
int launch_diff_p_sample(const float *x, const float *model_out, const float *noise, const long long *t,
                         const float *ra, const float *rb, const float *c1, const float *c2, const float *sigma, int T,
                         size_t B, size_t n, int param, int clip, float *out, float *x0_out, hipStream_t st);
int launch_diff_loss_sums(const float *pred, const float *target, size_t B, size_t n, int kind, void *workspace,
                          hipStream_t st);
int launch_diff_loss_finish(const void *workspace, const long long *t, const float *p2, const float *logvar,
                            const float *lvlb, int T, size_t B, size_t n, double lsw, double elbo, double *sums_out,
                            double *scalars_out, double *coef_out, double *dlogvar_out, hipStream_t st);
int launch_diff_loss_grad(const float *pred, const float *target, const float *grad_x0, const long long *t,
                          const float *rb, int T, const float *g, const double *coef, size_t B, size_t n, int kind,
                          float *grad_pred, hipStream_t st);
int launch_diff_canvas_gather(const float *src, const int *tiles, int ntiles, int B, int C, int h, int w, int ts,
                              float *out, hipStream_t st);
int launch_diff_canvas_stitch(const float *preds, int n_preds, int bstep, const int *tiles, int ntiles,
                              const double *weights, size_t wsb, size_t wsc, int B, int C, int h, int w, int ts,
                              float *out, hipStream_t st);

// ---- ssg_featmetric.hip: the LPIPS and DISTS criteria over a ragged set of feature pairs (entry points beside its
// kernels, where the layer records are built) ----
namespace featmetric {
struct LpipsSet;
struct DistsSet;
}  // namespace featmetric
int featmetric_grid_cap();
int featmetric_unit();
int featmetric_chunk();
int launch_lpips_layers(const featmetric::LpipsSet &s, void *workspace, double *out, hipStream_t st);
int launch_dists_score(const featmetric::DistsSet &s, const float *alpha, const float *beta, void *workspace, double *out,
                       hipStream_t st);

// ---- ssg_blindsr.hip: BSRGAN's degradation chain on a ragged batch, one launch per operation family (entry points
// beside its kernels) ----
int blindsr_grid_cap();
int launch_blindsr(int family, const void *table, int n_tiles, const float *in, float *out, const float *field,
                   const float *pool, hipStream_t st);

// ---- ssg_resample.hip: Pillow's 8-bit convolution resize (entry points beside its kernel) ----
int resample_ksize(int in, int out, int filter);                                   // host only
int resample_table(int in, int out, int filter, int *bounds, int *coef);           // host only: fp64, libm's sin / cos
void resample_tile_shape(int *th, int *tw);
int resample_max_ratio();
int launch_resample(const uint8_t *src, int B, int C, int Hin, int Win, int Hout, int Wout, int filter,
                    const int *xbounds, const int *xcoef, const int *ybounds, const int *ycoef, int out_kind, void *out,
                    hipStream_t st);

// ---- ssg_imresize.hip: MATLAB's bicubic imresize in fp64 (entry points beside its kernel) ----
int imresize_out_size(int n, double scale);                                        // host only
int imresize_taps(double scale, int antialias);                                    // host only
int imresize_table(int n, int m, double scale, int antialias, int *first, double *weights);   // host only: fp64
int imresize_tiles(double scale, int antialias, int *tiles, int capacity, int *chosen);
int launch_imresize(const void *src, int in_kind, int B, int C, int Hin, int Win, double scale, int antialias,
                    const int *yfirst, const double *yweights, const int *xfirst, const double *xweights, int out_kind,
                    void *out, hipStream_t st);

// ---- ssg_jpegcodec.hip: libjpeg's baseline round trip in integers (entry points beside its kernels) ----
size_t jpeg_roundtrip_workspace_bytes(int B, int H, int W, int channels);
int jpeg_unit_table(float *table);                                                 // host only
int launch_jpeg_roundtrip(const void *in, void *out, int B, int H, int W, int channels, const int *qualities,
                          int in_layout, int out_epilogue, void *workspace, size_t workspace_bytes, hipStream_t st);

// ---- ssg_api.hip ----
// host-mapped {rows for the direct kernels, dense tiles} of the device's last plan, written by the edge-list builder's
// scan kernel (nullptr: no hint wanted, or none allocated yet and `st` is being captured)
int *plan_hint_device_word(hipStream_t st);

}  // namespace ssg
