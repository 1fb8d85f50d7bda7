/*
 * ssg_hip.h -- C ABI of the MI355X (gfx950) Self-Similarity-Graph loss engine.
 *
 * This is the drop-in boundary for the ONE hot path of ChrisDud0257/SSL: the
 * SSG loss.  Everything below is `extern "C"`, takes
 * plain DEVICE pointers and sizes, allocates nothing, never synchronises the
 * host, and launches on the hipStream_t the caller passes (pass
 * torch.cuda.current_stream().cuda_stream from PyTorch).  All floating point
 * is IEEE fp32; indices are int32.
 *
 * Stream semantics: everything a call queues is ordered after the work already on
 * `stream` and before whatever the caller queues on `stream` next.  Inside a call
 * the direct kernel of a forward / backward pass (k_s <= 25) runs on a library-owned
 * side stream beside the dense-tile kernel, forked from and joined back into
 * `stream` with events -- invisible to the caller, and a stream capture of `stream`
 * records it as two parallel graph branches.  SSG_OVERLAP=0 (environment, read at
 * first use) keeps every launch on `stream` itself.
 *
 * Reference interface each group replaces (paths relative to
 * /root/reference/GAN-Based-SR/):
 *   (A) ssg_compute_similarity[_backward]   <- basicsr/losses/similarity/similarity.h:2-23
 *                                              (kernels similarity.cu:6-54, 74-131; pybind
 *                                              glue similaritywrapper.cpp:9-72)
 *   (B) ssg_edge_*                          <- scripts/data_preparation/generate_mask.py:22-31,
 *                                              torch.where / torch.nonzero in loss_util.py:196 and
 *                                              similaritywrapper.py:64-68, mask_stride pattern
 *                                              realesrganssl_model.py:64-72
 *   (C) ssg_map_forward / ssg_map_backward  <- similarity_map.ssl_pytorch / ssl_cuda,
 *                                              basicsr/losses/loss_util.py:182-244 (+ autograd)
 *   (D) ssg_loss_*                          <- the caller loop realesrganssl_model.py:379-430
 *                                              with L1Loss (basic_loss.py:41-66) and
 *                                              KLDistanceLoss (basic_loss.py:269-282)
 *   (E) ssg_augment_crop / ssg_pool_swap    <- basicsr/data/transforms.py:93-219 (joint flip/rot90 + crop of
 *                                              image and mask), realesrganssl_model.py:327-367 (pair pool)
 *
 * Return value of every int function: 0 on success, a positive hipError_t
 * from the launch, or a negative SSG_E_* code.  ssg_status_string() maps both.
 */
#ifndef SSG_HIP_H
#define SSG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ssg_stream_t; /* hipStream_t */

#define SSG_E_BADARG (-1)     /* null pointer, even / non-positive kernel size, k_w > k_s ...   */
#define SSG_E_TOOLARGE (-2)   /* search tile does not fit the 160 KiB LDS of a CU               */
#define SSG_E_WORKSPACE (-3)  /* caller's workspace is smaller than ssg_loss_workspace_bytes()   */
#define SSG_E_IMAGESMALL (-4) /* H or W <= k_s/2: reflect padding undefined (torch raises too)   */
#define SSG_E_ALIGN (-5)      /* fused step: workspace / grad_fix / grad_sr not 16-byte aligned      */
#define SSG_E_PLAN (-6)       /* ssg_device_status(): a plan cut for another tile height was used   */

/* 4 (round 4): + ssg_device_status, ssg_criteria_sums / _grad / _scratch_bytes, SSG_E_ALIGN, SSG_E_PLAN; a fused step
 * whose edge count exceeds its capacity returns NaN losses; a plan of the wrong tile height no longer traps. */
/* 5 (round 5): + ssg_set_overlap (modes 0-3, default 3 = per pass from the last plan's shape), ssg_last_overlap_assignment;
 * the product library no longer reads ANY environment variable (SSG_DENSE_THR, SSG_OVERLAP, SSG_OP_PLAN_FROM ... are
 * honoured by the profiling build only); the one-wave tile-major dense backward is gone. */
/* 6 (round 6): + ssg_set_tiny_step; default dense threshold 16. */
/* 6, additive: + ssg_ldl_workspace_bytes, ssg_artifact_map, ssg_artifact_map_backward, ssg_ldl_loss, ssg_local_variance
 * (LDL's artifact map, section (F)); nothing existing changed, so the version number stays. */
/* 6, additive: + ssg_bbl_workspace_bytes, ssg_bbl_search, ssg_bbl_loss, ssg_flat_mask (BebyGAN's best-buddy loss and
 * flat mask, section (G)); again nothing existing changed. */
/* 6, additive: + ssg_synth_kernels and its record (the degradation chain's blur and sinc kernels, section (I)). */
/* 6, additive: + ssg_resample, ssg_resample_table / _ksize / _tile / _max_ratio (Pillow's 8-bit resize, section (N)). */
/* 6, additive: + ssg_imresize, ssg_imresize_out_size / _taps / _table / _tiles (MATLAB's bicubic imresize, section (O)). */
/* 6, additive: + ssg_jpeg_roundtrip, ssg_jpeg_roundtrip_workspace_bytes, ssg_jpeg_unit_table (libjpeg's baseline round
 * trip, section (P)); nothing existing changed, so the version number stays. */
/* 6, additive: + ssg_gan_sums, ssg_gan_grad, ssg_gan_workspace_bytes, ssg_gan_grid_cap (the GAN criteria, section (Q)). */
/* 6, additive: + ssg_spsr_map, ssg_spsr_map_backward, ssg_spsr_loss, ssg_spsr_loss_backward, ssg_spsr_branch_loss,
 * ssg_spsr_branch_grad, ssg_pixel_sums, ssg_pixel_grad, ssg_spsr_workspace_bytes, ssg_spsr_grid_cap (SPSR's gradient map
 * and the pixel criteria, section (R)). */
/* 6, additive: + ssg_multi_apply, ssg_multi_table_fill, ssg_multi_table_bytes, ssg_multi_chunks, ssg_multi_chunk,
 * ssg_multi_grid_cap (the EMA and copy updates of a parameter set in one launch, section (S)). */
/* 6, additive: + ssg_mcrit_sums, ssg_mcrit_grad, ssg_mcrit_workspace_bytes, ssg_mcrit_chunk, ssg_mcrit_grid_cap and
 * SSG_PIX_FRO (a pixel criterion over a ragged set of tensor pairs: the perceptual loss, section (U)). */
/* 6, additive: + ssg_lpips_layers, ssg_dists_score, ssg_lpips_workspace_bytes, ssg_dists_workspace_bytes,
 * ssg_featmetric_grid_cap / _unit / _chunk (the LPIPS and DISTS criteria over their feature pairs, section (V)). */
/* 6, additive: + ssg_lpips_layers_backward (the LPIPS criterion's gradient with respect to both feature maps, section (V)). */
/* 6, additive: + ssg_diff_combine, ssg_diff_p_sample, ssg_diff_loss_sums, ssg_diff_loss_finish, ssg_diff_loss_grad,
 * ssg_diff_canvas_gather, ssg_diff_canvas_stitch, ssg_diff_workspace_bytes, ssg_diff_chunk, ssg_diff_grid_cap and
 * SSG_DIFF_EPS / _X0 / _V (the Diffusion fork around its network, section (W)). */
/* 6, additive once more: + ssg_adam_apply, ssg_adam_table_fill, ssg_adam_grads_fill, ssg_adam_table_bytes, the record
 * ssg_adam_scalars and SSG_ADAM_PLAIN / _L2 / _DECOUPLED (the Adam and AdamW step of a parameter group in one launch,
 * section (X)). */
/* 6, additive once more: + ssg_sn_forward, ssg_sn_backward, ssg_sn_table_fill, ssg_sn_table_bytes, ssg_sn_output_bytes,
 * ssg_sn_workspace_bytes, ssg_sn_saved_bytes, ssg_sn_chunk, ssg_sn_grid_cap, ssg_sn_strip, ssg_sn_rows_a, ssg_sn_rows_b
 * (spectral normalisation of a layer set in a fixed handful of launches, section (Y)). */
/* 6, additive once more: + ssg_winattn_forward, ssg_winattn_backward, ssg_winattn_workspace_bytes, ssg_winattn_grid_cap
 * (SwinIR's shifted-window attention between the qkv and proj Linears, section (Z)). */
int ssg_abi_version(void);
const char *ssg_status_string(int status);
/* Device-side refusals that no return value can carry (everything is asynchronous): waits for `stream`, then returns
 * SSG_E_PLAN if, since the last call, a dense-tile kernel of ssg_map_forward / ssg_map_backward / ssg_loss_backward was
 * handed a fwd_plan cut for another tile height than its k_s uses (ssg_edge_list's plan_ks: 8-row tiles for k_s <= 25,
 * 4-row tiles for k_s = 49) -- such a launch leaves its rows / gradient untouched instead of decoding tile ids with
 * the wrong geometry -- else 0.  Clears the word.  The status word (4 bytes per device) is the one thing the library
 * allocates, at the first forward / backward call that takes a plan.  ssg_loss_fwd_bwd / ssg_loss_step build their own
 * plan and cannot set it. */
int ssg_device_status(ssg_stream_t stream);

/* ---------------------------------------------------------------- (A) ----
 * Reference operator, same argument meaning as similarity.h:2-11 plus a
 * stream and a status.  `image` is the REFLECT-PADDED (channel,height,width)
 * fp32 image, `pos` holds mc (Y,X) int32 pairs in PADDED coordinates, `out`
 * is (mc,psize,psize) and is ACCUMULATED into (the reference kernel does
 * `out[...] += d*d` on a zeroed buffer).  Raw squared patch distances, no
 * epilogue.  Asynchronous. */
/* Calls with many positions build the engine's work split inside the call: from ssg_set_operator_plan_threshold()
 * positions on for the backward and three times as many for the forward (default 8192 / 24576; n <= 0: never; 1:
 * always, both; environment SSG_OP_PLAN_FROM) and for the sizes that have shared-term
 * kernels ((25,9,3), (49,13,3)) the position list becomes a rank map and a plan -- the buffers come from a
 * library-owned, stream-ordered memory pool (hipMallocFromPoolAsync / hipFreeAsync on `stream`: the reference interface
 * has no workspace argument) -- and the tiles holding many positions go through the shared-term kernels, the others
 * through the direct kernels in tile order; `pos` may be in any order and may repeat positions (each row is still
 * computed).  Same results either way (raw distances rel 2e-6).  Below the threshold, and inside a stream capture,
 * the direct kernels walk `pos` as it comes.  Measured, launches only (profiles/r4_operator_plan_path.txt): 4,697
 * positions forward 0.056 ms direct / 0.206 with the plan, backward 0.158 / 0.167; 18,417 positions forward 0.196 /
 * 0.231, backward 0.462 / 0.258.  Returns the previous threshold. */
int ssg_set_operator_plan_threshold(int positions);
/* The pool keeps what the largest call needed (mask, rank map, plan: ~24 bytes per padded pixel + 20 per position; the
 * backward's scratch: 4 k_s^2 bytes per position) so that later calls allocate without a system call;
 * ssg_operator_pool_trim() hands the unused part back to the driver (after the work that used it has finished). */
int ssg_operator_pool_trim(void);
int ssg_compute_similarity(const float *image, const int *pos, float *out,
                           int mc, int psize, int ksize, int height, int width,
                           int channel, ssg_stream_t stream);

/* similarity.h:13-23: scatter of `grads` = dL/d(out) (mc,psize,psize) into
 * `image_grads` (channel,height,width, PADDED layout, accumulated into).  The
 * reference uses ~2*C*ksize^2 global atomics per (edge pixel, offset); this
 * one reduces per edge pixel on chip and issues one atomic per touched
 * pixel. */
int ssg_compute_similarity_backward(const float *image, const float *grads,
                                    const int *pos, float *image_grads, int mc,
                                    int psize, int ksize, int height, int width,
                                    int channel, ssg_stream_t stream);

/* ---------------------------------------------------------------- (B) ----
 * Edge list of a batch, built on device without a host round trip.
 *
 * mask_kind: 0 = fp32 mask (B,mask_channels,H,W), an edge pixel is
 *                `mask[b,0,y,x] == 1.0f` (loss_util.py:196 on channel 0, like
 *                ssl_cuda's mask[0,0], loss_util.py:233);
 *            1 = uint8 mask, same layout, `== 1` (a 0/255 PNG mask must be
 *                divided by 255 first, exactly as for the reference's
 *                `mask == 1`);
 *            2 = no mask tensor: `mask` is the fp32 GT batch (B,3,H,W) in
 *                [0,1] and the reference's offline mask is generated on the
 *                fly: u8 = round(255 x), L = PIL 'L' (ITU-R 601-2 16.16 fixed
 *                point), 4-neighbour Laplacian with BORDER_REFLECT_101
 *                saturated to uint8, `> lap_threshold` (generate_mask.py:22-31).
 * mask_stride > 1 additionally keeps only y % s == x % s
 * (realesrganssl_model.py:64-72).
 *
 * Outputs: edges  (capacity,3) int32 rows (b,y,x) in UNPADDED coordinates,
 *                 ordered by image then row-major -- the order of
 *                 torch.cat([...], dim=1) over torch.where;
 *          counts (B+2) int32: counts[0] = total N (NOT clamped to capacity;
 *                 N > capacity means overflow: re-run with a larger list),
 *                 counts[1+b] = first row of image b, counts[1+B] = N.
 *          rank_map (nullable) (B,H,W) int32: for every pixel the row of
 *                 `edges` that holds it, or -1.
 *          tile_order (nullable, needs rank_map) (capacity) int32: the rows
 *                 0..N-1 permuted tile-major (8x8 image tiles, row-major
 *                 inside a tile).  Passing it to the backward entry points
 *                 makes consecutive jobs spatial neighbours, whose gradient
 *                 tiles are then summed on chip before touching HBM (3.5x
 *                 fewer global atomics).  Rows of the SSG tensors keep the
 *                 reference's order either way.  Entries hold the row in bits
 *                 0..29; bit 30 of every 5th entry (first of a group of five
 *                 jobs) marks groups whose edge pixels share one image and an
 *                 8 x 16 pixel window (the kernels' on-chip sharing test).
 *          fwd_plan (nullable, needs rank_map) ssg_forward_plan_bytes() bytes:
 *                 the forward's work split -- 8x32-pixel tiles holding at
 *                 least ssg_set_dense_threshold() edge pixels go to the
 *                 shared-term ("dense") kernels, the remaining rows, in their
 *                 own tile-major order, to the direct kernels.  The plan records
 *                 its own split (with threshold 0: no dense tile, every row in
 *                 the direct order), so its consumers never read the process-wide
 *                 threshold.  Kernel sizes other than (25, 9, C=3) ignore it.
 * scratch: ssg_edge_scratch_bytes(B,H,W) bytes of device memory. */
size_t ssg_edge_scratch_bytes(int B, int H, int W);
size_t ssg_forward_plan_bytes(int B, int H, int W, int capacity);
/* Threshold (edge pixels per 8x32 tile) from which the forward routes a tile to the
 * shared-term kernel; 0 = never.  Default 16.  Results are the same either way (parity-tested
 * with every tile routed through it and with none).  Process-wide; takes effect at the
 * next ssg_edge_list().  Returns the previous value.  No reference counterpart: the
 * reference has one code path. */
int ssg_set_dense_threshold(int edge_pixels_per_tile);
/* Stream assignment of the two kernels of a pass for k_s <= 25 (a library-owned side stream, event fork / join on the
 * caller's stream; capturable).  0: every launch on the caller's stream (per-kernel profiling).  1: the dense-tile
 * kernel on the caller's stream, the direct kernel beside it on the side stream -- for masks whose dense tiles carry
 * most rows (Laplacian edge masks).  2: the other way round -- for masks without dense tiles (Bernoulli, thin strided
 * masks: the whole critical path on one stream; Bernoulli 1 % -15 %, C2 +3 %).  3 (default): 1 or 2 per call, by the
 * shape of the last plan ssg_edge_list / the fused step built on the device -- its scan kernel leaves {rows for the
 * direct kernels, dense tiles} in host-mapped memory, the host reads it at the next pass without synchronising; the
 * branch expected to take longer (38 ns per direct row against 0.74 us per dense tile) stays on the caller's stream.
 * In mode 3 the fused steps (ssg_loss_fwd_bwd, ssg_loss_step) also run forward AND backward of the two branches as two
 * chains with ONE join at the end: free-running when the direct chain carries the step or the plan holds at most 512
 * dense tiles, otherwise with the direct backward held by a one-way event until the dense forward is through (C2 1.27 ->
 * 1.25 ms, C4 0.50 -> 0.46, Bernoulli 1 % 0.185 -> 0.175).
 * Same results, bit for bit in deterministic mode, in every mode and schedule (disjoint rows, integer sums at a scale that
 * does not depend on the schedule).  Process-wide; returns the previous setting.  No reference counterpart (the
 * reference launches on the legacy stream, similarity.cu:69,147). */
int ssg_set_overlap(int mode);
/* Diagnostics: the assignment the calling thread's last forked pass used (0 not forked, 1, 2 as above). */
int ssg_last_overlap_assignment(void);
/* Small fused steps.  ssg_loss_fwd_bwd / ssg_loss_step at (k_s, k_w, C) = (11, 5, 3) -- BASELINE's configs[0], the
 * reference's own CPU-runnable case (loss_util.py:185-229 on a 64 x 64 crop) -- with B*H*W <= 16,384 pixels and
 * capacity <= 4,096 rows run as TWO launches: one workgroup builds the edge list and clears the sums, then one workgroup
 * per edge pixel computes both SSG rows, the criteria and the row's gradient, and the last one through folds the step
 * (ssg_tiny.hip; C1: 59 -> 27 us).  Same outputs, workspace and error behaviour as the general path; results equal
 * to rounding (other summation orders), bit-reproducible in deterministic mode.  The workspace then holds the edge list and
 * the rank map but no tile order.  on = 0 keeps every call on the general path (default 1).  Process-wide; returns the
 * previous setting.  No reference counterpart. */
int ssg_set_tiny_step(int on);
int ssg_edge_list(const void *mask, int mask_kind, int mask_channels, int B,
                  int H, int W, int mask_stride, float lap_threshold,
                  int plan_ks /* k_s the fwd_plan is built for (tile rows: 8, or 4 for k_s = 49); 0 = 25.
                               * CONSTRAINT: a plan is only valid for calls whose k_s uses the same tile height --
                               * the plan records it (fwd_plan[2]) and the dense kernels of ssg_map_forward /
                               * ssg_map_backward / ssg_loss_backward do NOTHING when it differs from theirs
                               * (ssg_device_status() then returns SSG_E_PLAN), instead of decoding tile ids with
                               * the wrong geometry.  ssg_loss_fwd_bwd builds its own plan and cannot get this wrong. */,
                  int *edges, int capacity, int *counts,
                  int *rank_map /* nullable */, int *tile_order /* nullable */,
                  int *fwd_plan /* nullable */, void *scratch,
                  ssg_stream_t stream);

/* The mask itself (B,H,W) uint8 {0,1} from an fp32 GT batch (B,3,H,W):
 * mask_kind 2 above materialised (offline tool generate_mask.py). */
int ssg_edge_mask_laplacian(const float *gt, int B, int H, int W,
                            float lap_threshold, int mask_stride,
                            uint8_t *mask_out, ssg_stream_t stream);

/* ---------------------------------------------------------------- (C) ----
 * similarity_map forward for a batch of UNPADDED images (B,C,H,W) (reflect
 * padding is done by index mirroring, nothing is materialised):
 *   D  = patch distances, q = D/(C*k_w^2), e = exp(-1*q/sigma),
 *   s  = generalization ? 1/(sum_p e + eps) * e : e        (loss_util.py:224-227)
 * `edges` as produced by ssg_edge_list; n_edges_dev (nullable) points at the
 * device-side row count (counts[0]); at most n_rows rows are computed (the
 * host-known bound used to size the launch and `ssg`).  ssg is (n_rows,
 * k_s*k_s) fp32, row n <-> edges[n].  If img2/ssg2 are non-null the same
 * edge list is evaluated on a second batch in the same launch (SR and GT).
 * tile_order (from ssg_edge_list) only changes which workgroup computes which
 * row: neighbouring edge pixels then share one LDS search region.
 * With a fwd_plan, n_rows must cover the rows the plan was cut for: n_rows >= min(counts[0], capacity of the
 * ssg_edge_list call) -- the launches over the plan's heavy tiles are sized from n_rows (a heavy tile holds more than
 * 64 rows).  The same holds for ssg_map_backward / ssg_loss_backward. */
int ssg_map_forward(const float *img, const float *img2, int B, int C, int H,
                    int W, const int *edges, const int *tile_order /* nullable */,
                    const int *rank_map /* nullable */,
                    const int *fwd_plan /* nullable */,
                    const int *n_edges_dev, int n_rows,
                    int ks, int kw, float sigma, float eps, int generalization,
                    float *ssg, float *ssg2,
                    double *row_scale /* nullable, 2*n_rows doubles: see ssg_loss_backward */,
                    ssg_stream_t stream);

/* Backward of the above: grad_img (B,C,H,W) += d/d img of sum(grad_ssg * ssg)
 * (reflect fold included).  `ssg` is the forward output (saved).
 * With rank_map, fwd_plan (both from ssg_edge_list) and `scratch`
 * (ssg_backward_scratch_bytes(n_rows, ks) bytes) the backward is split like
 * the forward: dL/dD rows are formed once (ssg_grad_rows), the plan's dense
 * tiles go through the shared-term backward kernel and the remaining rows
 * through the direct one.  Any of the three null: direct kernel for every row. */
size_t ssg_backward_scratch_bytes(int n_rows, int ks);
int ssg_map_backward(const float *img, int B, int C, int H, int W,
                     const int *edges, const int *tile_order /* nullable */,
                     const int *rank_map /* nullable */,
                     const int *fwd_plan /* nullable */,
                     const int *n_edges_dev, int n_rows,
                     int ks, int kw, float sigma, int generalization,
                     const float *ssg, const float *grad_ssg, float *grad_img,
                     void *scratch /* nullable */, void *grad_fix /* nullable */,
                     ssg_stream_t stream);

/* Deterministic gradient accumulation.  By default the kernels add their per-pixel contributions to the image
 * gradient with hardware fp32 atomics: the order of the additions, hence the last bits of the result, varies
 * from run to run (as with the reference's atomicAdd, similarity.cu:123-128).  Passing `grad_fix` --
 * ssg_grad_fix_bytes(B,C,H,W) bytes of device memory, contents irrelevant -- to the backward entry points makes
 * the result bit-reproducible: contributions are rounded to multiples of a power of two chosen on the device
 * from an upper bound of |dL/dD| over the call (2^-35 of it; headroom for pixel differences up to 16) and summed
 * with 64-bit integer atomics (integer addition is associative), then folded into grad once per pixel.  The bound:
 * ssg_map_backward and the k_s = 49 tile-major step take the exact maximum (11 bits finer than an fp32 sum of the same
 * terms); the loss steps take the a-priori bound 4 (|w_l1| u_1 + |w_kl| u_2) / (sigma C k_w^2 n k_s^2) -- |s g| <= w_1 +
 * w_2 because s, t <= 1 -- which needs no pass over the rows and does not depend on how the step is scheduled
 * (ssg_set_overlap).  It lies further above the maximum the flatter the rows are; measured at sigma 0.004, 0.05 and 1,
 * (25,9) and (11,5): the deterministic gradient stays within 2e-7 max|grad| of the fp32-atomic one, which is the atomics'
 * own run-to-run spread (tools/r5_fix_resolution.py). */
size_t ssg_grad_fix_bytes(int B, int C, int H, int W);

/* ---------------------------------------------------------------- (D) ----
 * The whole loss step of the caller loop over a batch:
 *   l1 = w_l1 * mean |s_sr - s_gt|,  kl = w_kl * mean t'(log t' - log s')
 * with the mean over M = N * k_s^2 elements of the LOCAL batch (images with
 * an empty mask contribute nothing; N == 0 gives 0,0 like ddpmssl.py:492),
 * and grad_sr (B,C,H,W) += d(l1+kl)/d sr.
 *
 * ssg_loss_backward consumes SSGs already computed by ssg_map_forward
 * (API-compatible mode: SSG tensors are materialised once each); rank_map and
 * fwd_plan (nullable, from ssg_edge_list) select the split backward described
 * at ssg_map_backward (its scratch is part of ssg_loss_scratch_bytes).
 * Deferred normalisation (optional): when the SAME `row_scale` buffer (2*n_rows doubles) is passed to
 * ssg_map_forward and then here, the rows the dense-tile forward produced are left un-normalised
 * (e = exp(-d/sigma)) with their 1/(sum e + eps) in row_scale, and this call rescales them in place while it
 * streams them anyway -- same arithmetic, same bits, one pass over the SSG tensors less.  Between the two calls
 * ssg_sr / ssg_gt are NOT yet the SSG tensors.  Requires rank_map, fwd_plan and scratch (SSG_E_BADARG otherwise).
 * rows_are_scratch != 0: the caller will not look at ssg_sr / ssg_gt again (an autograd node that keeps only the
 * gradient): the rescaled rows are then not written back -- one write of every deferred row less.
 * `upstream`
 * (nullable) points at two DEVICE floats {dL/dl1, dL/dkl} that scale the two
 * criteria's gradients (autograd's incoming gradients, read on device so the
 * host never synchronises); null means {1,1}.
 * loss_out: 2 floats {l1, kl} on device.  scratch: ssg_loss_scratch_bytes(B,H,W,n_rows,ks).
 * PRECONDITION of the deterministic mode (grad_fix != NULL) at k_s <= 25: the rows are SSG rows -- every entry of
 * ssg_sr / ssg_gt in [0, 1] and every ssg_gt row summing to at most 1 (true for whatever ssg_map_forward produces,
 * normalised or not).  The fixed-point scale of the gradient sums is then taken from the a-priori bound
 * |dL/dD| <= 4 (|w_l1| u_1 + |w_kl| u_2) / (sigma C k_w^2 n k_s^2) instead of a maximum over the rows (no reduction
 * pass); rows outside those ranges (foreign tensors) can exceed the bound and wrap the 64-bit sums silently -- pass
 * grad_fix = NULL (fp32 atomics) for such input.  k_s = 49 with tile-major rows keeps the exact maximum. */
size_t ssg_loss_scratch_bytes(int B, int H, int W, int n_rows, int ks);
int ssg_loss_backward(const float *sr, int B, int C, int H, int W,
                      const int *edges, const int *tile_order /* nullable */,
                      const int *rank_map /* nullable */,
                      const int *fwd_plan /* nullable */,
                      const int *n_edges_dev, int n_rows,
                      int ks, int kw, float sigma, int generalization,
                      float *ssg_sr, float *ssg_gt, float w_l1,
                      float w_kl, const float *upstream /* nullable */,
                      float *loss_out, float *grad_sr /* nullable */,
                      void *scratch, void *grad_fix /* nullable: deterministic mode */,
                      const double *row_scale /* nullable */, int rows_are_scratch, ssg_stream_t stream);

/* The two criteria on tensors that already exist (L1Loss basic_loss.py:41-66 with l1_loss :14-16; KLDistanceLoss
 * basic_loss.py:269-282): sums_out[0] = sum |pred - target|, sums_out[1] = sum t' (log t' - log s') with
 * s' = max(pred, 1e-10), t' = max(target, 1e-10), over n fp32 elements, in one streaming pass (fp64 accumulation in a
 * fixed order: bit-reproducible); the caller applies reduction and loss_weight (mean = sum / n).  `scratch`:
 * ssg_criteria_scratch_bytes() bytes.  ssg_criteria_grad: grad_pred[i] = coef[0] * sign(pred - target) - coef[1] *
 * t'/s' (second term 0 where pred < 1e-10: the clamp's derivative), coef = 2 DEVICE floats (the upstream gradients
 * times weight / n: no host round trip).  The engine's fused entry points below compute the same terms inside their
 * row passes; these two serve SSG tensors that were materialised (eager `similarity_map`, INTEGRATION.md Level 1). */
size_t ssg_criteria_scratch_bytes(void);
int ssg_criteria_sums(const float *pred, const float *target, size_t n, void *scratch, float *sums_out,
                      ssg_stream_t stream);
int ssg_criteria_grad(const float *pred, const float *target, size_t n, const float *coef, float *grad_pred,
                      ssg_stream_t stream);

/* Everything in one call: edge list (from a mask or from GT's Laplacian),
 * SSG(sr), SSG(gt), both criteria and the gradient.  ssg_sr / ssg_gt
 * (capacity, k_s*k_s) receive the SSG tensors; `counts` as in ssg_edge_list;
 * workspace >= ssg_loss_workspace_bytes(B,H,W,capacity,ks).
 * ALIGNMENT: `workspace`, `grad_fix` and `grad_sr` must be 16-byte aligned (SSG_E_ALIGN otherwise): the edge-list
 * builder's first kernel clears the row scales, the fixed-point sums and (ssg_loss_step) the gradient with 16-byte
 * stores.  Fresh allocations are; an offset view into a larger buffer has to keep the alignment.
 * OVERFLOW: counts[0] > capacity means the step has used the first `capacity` edge pixels only; loss_out is then
 * {NaN, NaN}, so that a truncated step cannot pass for a complete one (grad_sr holds the truncated step's gradient).
 *
 * Fused step, no SSG output (SURVEY 8d's B_alg' mode): ssg_sr == ssg_gt == NULL.  The rows then live in the
 * workspace, which must hold ssg_loss_workspace_bytes(...) + ssg_loss_rows_bytes(capacity, ks); the dense-tile
 * forward leaves them un-normalised, ssg_grad_rows reads them once (rescaling in registers) and nothing normalised is
 * ever written -- one write and one read of every row instead of two writes and two reads (C5: 26 -> 21 GB per step).
 * Loss and gradient are bit-identical to the materialising call (row-major rows).  A kernel that kept a tile's rows
 * on chip through criteria and backward would need 64 edge pixels x k_s^2 x 2 images x 4 B = 320 KB at (25,9) --
 * twice the LDS of a CU -- or a second forward sweep; DESIGN.md section 8 has the measured costing.
 *
 * k_s = 49 (k_w 13, C 3, generalization): ssg_loss_rows_bytes() holds a second pair of regions for TILE-MAJOR rows,
 * [slot of the plan's dense-tile list][offset q][128 pixels of the 4 x 32 tile].  A call whose dense tiles fit the
 * region (count <= capacity / 128) and are >= 60 % full on average -- decided on the device from the plan's counts,
 * for all tiles of the call or none -- keeps the dense tiles' rows there: the forward stores whole 256-byte runs,
 * ssg_rows_tm reads them once (criteria, sum_q g s, border sums), and the dense backward forms G = dL/dD itself
 * from the two rows instead of reading G rows (C5: 21 -> 15.7 GB per step, 7.7 -> 5.7 ms); whole strips of nine heavy
 * tiles (36 x 32 pixels, consecutive slots) get their forward rows from ssg_fwd_strip.  Same loss and gradient as the
 * row-major step up to fp32 rounding: l1 <= 2e-7, kl <= 5e-6 relative; the gradient is within 5e-7 of the fp64
 * oracle's like the row-major step's, and within 4e-5 of its maximum of the row-major step's (the strip forward
 * rounds e differently, and a few L1 entries whose sign(s_sr - s_gt) fp32 does not decide flip).  Bit-reproducible
 * run to run in deterministic mode.  SSG_TILE_MAJOR=0 (environment) keeps every row row-major, SSG_STRIPS=0 leaves
 * the forward to the tile kernel.
 * A MATERIALISING k_s = 49 call (ssg_sr / ssg_gt given) uses the tile-major rows too when its workspace holds
 * ssg_loss_workspace_bytes() + ssg_loss_tm_bytes(): forward and backward as above, and the row pass
 * (ssg_rows_tm_mat) also writes the normalised SSG rows into the caller's tensors, 196-byte runs at a time.
 * ssg_loss_workspace_layout() reports where the pieces of the workspace live (byte offsets; `fused` = 1 for a call
 * without SSG output; tests and tools read the scratch rows of a finished call through it): out[0] edge list, [1]
 * rank map, [2] plan, [3] row scales (2 x capacity doubles, negative = tile-major row), [4] / [5] row-major scratch
 * rows of sr / gt (fused only), [6] / [7] tile-major regions of sr / gt (0 when the size has none), out[8] = slots
 * of a tile-major region. */
size_t ssg_loss_workspace_bytes(int B, int H, int W, int capacity, int ks);
size_t ssg_loss_rows_bytes(int capacity, int ks);
size_t ssg_loss_tm_bytes(int capacity, int ks);
int ssg_loss_workspace_layout(int B, int H, int W, int capacity, int ks, int fused, size_t out[9]);
int ssg_loss_fwd_bwd(const float *sr, const float *gt, const void *mask,
                     int mask_kind, int mask_channels, int B, int C, int H,
                     int W, int ks, int kw, float sigma, float eps,
                     int generalization, float w_l1, float w_kl, int mask_stride,
                     float lap_threshold, int capacity, float *ssg_sr /* nullable with ssg_gt: fused step */,
                     float *ssg_gt, int *counts, float *loss_out, float *grad_sr,
                     void *workspace, size_t workspace_bytes,
                     void *grad_fix /* nullable: deterministic mode */, ssg_stream_t stream);

/* ssg_loss_fwd_bwd with the gradient as an OUTPUT: grad_sr (B,C,H,W) is overwritten with d(l1+kl)/d sr instead of
 * accumulated into, so the caller does not clear it first (one fill kernel per step less: the deterministic mode's
 * final fold assigns it, the fp32-atomics mode has it cleared by the edge-list builder's first kernel).  Everything
 * else as ssg_loss_fwd_bwd.  N == 0 (every mask empty): grad_sr = 0. */
int ssg_loss_step(const float *sr, const float *gt, const void *mask,
                  int mask_kind, int mask_channels, int B, int C, int H,
                  int W, int ks, int kw, float sigma, float eps,
                  int generalization, float w_l1, float w_kl, int mask_stride,
                  float lap_threshold, int capacity, float *ssg_sr /* nullable with ssg_gt: fused step */,
                  float *ssg_gt, int *counts, float *loss_out, float *grad_sr,
                  void *workspace, size_t workspace_bytes,
                  void *grad_fix /* nullable: deterministic mode */, ssg_stream_t stream);

/* ---------------------------------------------------------------- (E) ----
 * The step before the loss, on the GPU (minimal slice): joint augmentation + crop of image and mask, and the
 * training pair pool.  Byte moves only, bit exact.
 *
 * ssg_augment_crop <- basicsr/data/transforms.py:152-219 `augment` (hflip, then vflip, then rot90 = transpose,
 * the same draw for image and mask) followed by transforms.py:93-149 `paired_random_crop_img_mask`: dst
 * (B,C,Ho,Wo) = crop at (top,left) of the augmented src (B,C,Hs,Ws); params (B,5) int32 on device:
 * top, left, hflip, vflip, rot90 per sample (top/left index the AUGMENTED image; the caller draws them like the
 * reference does and scales them for the GT side).  elem_bytes 4 (fp32 images / masks) or 1 (uint8 masks).
 *
 * ssg_pool_swap <- realesrganssl_model.py:327-367 `_dequeue_and_enqueue` for one tensor of the pool: samples
 * `slots[k]` of `queue` (Q samples of sample_bytes each) and sample k of `batch` change places, k < b. */
int ssg_augment_crop(const void *src, void *dst, int elem_bytes, int B, int C, int Hs, int Ws, int Ho, int Wo,
                     const int *params, ssg_stream_t stream);
int ssg_pool_swap(void *queue, void *batch, size_t sample_bytes, const int *slots, int b, ssg_stream_t stream);

/* USMSharp.forward (basicsr/utils/img_process_util.py:63-83; applied to every GT batch, realesrganssl_model.py:165,
 * 315): out = soft * clip(img + weight * (img - G*img), 0, 1) + (1 - soft) * img, soft = G * (|img - G*img| * 255 >
 * threshold), G = cv2.getGaussianKernel(radius | 1, sigma) x its transpose (sigma <= 0: OpenCV's rule 0.3 ((k-1)/2 -
 * 1) + 0.8), reflect padding.  img, out (B,C,H,W) fp32, out != img; H, W > radius / 2 (SSG_E_IMAGESMALL otherwise, as
 * F.pad raises); odd kernel size <= 63; scratch >= ssg_usm_scratch_bytes (3 planes of the batch).  Reference defaults:
 * radius 50, sigma 0, weight 0.5, threshold 10.  Floating point: within 2e-6 of the fp64 evaluation except where
 * |residual| * 255 is within rounding of `threshold` (the mask bit is then not determined at fp32). */
/* filter2D (basicsr/utils/img_process_util.py:7-31; the blur steps of the degradation chain,
 * realesrganssl_model.py:173,212,245,281,294): out[b,c] = reflect-padded img[b,c] correlated with kernels[b] (n_kernels
 * == B) or kernels[0] (n_kernels == 1); kernels (n_kernels, k, k) fp32, k odd <= 21 (ValueError for even k in the
 * reference: SSG_E_BADARG); H, W > k / 2; out != img.  Within 2e-6 of the fp64 evaluation for blur kernels (sum 1). */
int ssg_filter2d(const float *img, const float *kernels, float *out, int B, int C, int H, int W, int k, int n_kernels,
                 ssg_stream_t stream);
/* DiffJPEG(differentiable=False).forward (basicsr/utils/diffjpeg.py:449-487; realesrganssl_model.py:34,201,240,285,
 * 290): the JPEG simulation of the degradation chain on (B,3,H,W) fp32 RGB in [0,1] -- zero padding to multiples of
 * 16, YCbCr, 2x2 chroma average, 8x8 DCT, quantisation with torch.round at factor = quality_to_factor(quality),
 * inverse path, clamp, crop -- fused into one kernel (one wave per 16x16 macroblock).  quality_dev: B device floats
 * (the reference's tensor branch), or NULL to use the host scalar `quality` for every sample.  out may alias img.
 * Floating point: a DCT coefficient whose quotient lies within fp32 rounding of k + 1/2 may round the other way than in
 * another fp32 implementation (the reference's own included); everywhere else within 3e-6 of the fp64 evaluation. */
int ssg_diffjpeg(const float *img, float *out, int B, int H, int W, const float *quality_dev, float quality,
                 ssg_stream_t stream);
size_t ssg_usm_scratch_bytes(int B, int C, int H, int W);
int ssg_usm_sharp(const float *img, float *out, int B, int C, int H, int W, int radius, float sigma, float weight,
                  float threshold, void *scratch, size_t scratch_bytes, ssg_stream_t stream);

/* The element-wise / gather stages of the degradation chain (realesrganssl_model.py:168-297) between the kernels above
 * (ssl_amd/csrc/ssg_degrade.hip).  All take device pointers, launch on `stream`, never synchronise.
 *
 * ssg_resize: torch.nn.functional.interpolate(img, scale_factor=s | size=(Ho, Wo), mode) as the model calls it
 *   (:185,203,224,255,280,293; align_corners=False, antialias=False): mode 0 'area' (adaptive average pooling),
 *   1 'bilinear', 2 'bicubic' (A = -0.75).  scale_factor_h / _w: the scale_factor the caller would have passed to
 *   F.interpolate (the source coordinates then use 1 / scale_factor like torch, not Hi / Ho), or 0 for the size= form;
 *   Ho, Wo are always given (floor(Hi * scale_factor) for the scale_factor form).  out != img. */
int ssg_resize(const float *img, float *out, int B, int C, int Hi, int Wi, int Ho, int Wo, int mode,
               double scale_factor_h, double scale_factor_w, ssg_stream_t stream);
/* clip && rounds: torch.clamp((x * 255.0).round(), 0, 255) / 255. (realesrganssl_model.py:206,297; round half to even);
 * clip only: clamp(x, 0, 1); rounds only: (x * 255).round() / 255 -- the tail of add_*_noise_pt, degradations.py:501-507. */
int ssg_clamp_round(const float *img, float *out, size_t n, int clip, int rounds, ssg_stream_t stream);
/* add_gaussian_noise_pt (basicsr/data/degradations.py:455-507) with the random fields passed in: field_color (B,C,H,W) =
 * the torch.randn(b,c,h,w) draw, field_gray (H,W) = the torch.randn(h,w) draw (one field for the whole batch, as the
 * reference's broadcast has it) or NULL when no sample has gray noise; sigma (B), gray (B) in {0,1} on the device. */
int ssg_gaussian_noise(const float *img, float *out, const float *field_color, const float *field_gray,
                       const float *sigma, const float *gray, int B, int C, int H, int W, int clip, int rounds,
                       ssg_stream_t stream);
/* add_poisson_noise_pt (degradations.py:601-674) around the torch.poisson draws.  ssg_poisson_rates: the per-sample
 * level census (the reference's torch.unique, a host loop there), vals = 2^ceil(log2(levels)) -> vals (B,2) =
 * (colour, gray), and the rates img_r * vals the draws are taken from (rate_gray (B,1,H,W) nullable: only when a
 * sample has gray noise; C must be 3 then).  ssg_poisson_noise: the arithmetic after the draws. */
size_t ssg_poisson_scratch_bytes(int B);
int ssg_poisson_rates(const float *img, float *rate_color, float *rate_gray, float *vals, void *scratch, int B, int C,
                      int H, int W, ssg_stream_t stream);
int ssg_poisson_noise(const float *img, float *out, const float *draw_color, const float *draw_gray, const float *vals,
                      const float *scale, const float *gray, int B, int C, int H, int W, int clip, int rounds,
                      ssg_stream_t stream);

/* ---------------------------------------------------------------- (F) ----
 * LDL's artifact map and loss (basicsr/losses/loss_util.py:106-161; callers ldlssl_model.py:220-224 and
 * realesrgan_model.py:222-226: pixel_weight = get_refined_artifact_map(gt, output, output_ema, 7), then
 * L1Loss(pixel_weight * output, pixel_weight * gt)), ssl_amd/csrc/ssg_ldl.hip.  output, gt, ema (B,C,H,W) fp32:
 *   r = sum_c |gt - output|, r_e = sum_c |gt - ema|, P_b = var_unbiased(r_b)^(1/5),
 *   V_p = unbiased variance of the k x k reflect-padded window of r around p,
 *   w = P_b V_p, set to 0 where r < r_e (ema non-null: get_refined_artifact_map; ema NULL: get_artifact_map).
 * k odd, 3 <= k <= 15 (7 is the compiled fast path); any C >= 1; H, W > (k-1)/2.  Status: SSG_E_BADARG for a null
 * pointer, k even or < 3, B, C, H or W <= 0; SSG_E_TOOLARGE for k > 15; SSG_E_IMAGESMALL for H or W <= (k-1)/2 (torch's
 * reflect pad raises); SSG_E_WORKSPACE for workspace_bytes < ssg_ldl_workspace_bytes(B, H, W); SSG_E_ALIGN for a
 * workspace that is not 16-byte aligned.  Three launches at
 * most, no atomics, fixed summation orders: results are bit-reproducible.  The gradient is with respect to `output`
 * only.  An image whose residual r is constant (output == gt) has var = 0; like the reference's pow backward (0 * inf)
 * its whole gradient is NaN.
 * ssg_artifact_map: w_out (B,1,H,W).
 * ssg_artifact_map_backward: grad_output (B,C,H,W) = d/d output of sum(grad_w * w) (overwritten).
 * ssg_ldl_loss: loss_out[0] = loss_weight * mean |w*output - w*gt| (mean != 0; the sum otherwise), the products rounded
 *   separately in fp32; grad_output (nullable) = d loss / d output (overwritten).
 * ssg_local_variance (get_local_weights): residual (B,1,H,W) planes taken as they are (no abs, no P, no mask):
 *   v_out (nullable) = V; with grad_v and grad_residual (both or neither) grad_residual = d/d residual of sum(grad_v V). */
size_t ssg_ldl_workspace_bytes(int B, int H, int W);
int ssg_artifact_map(const float *output, const float *gt, const float *ema /* nullable */, int B, int C, int H, int W,
                     int k, float *w_out, void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_artifact_map_backward(const float *output, const float *gt, const float *ema /* nullable */,
                              const float *grad_w, int B, int C, int H, int W, int k, float *grad_output,
                              void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_ldl_loss(const float *output, const float *gt, const float *ema /* nullable */, int B, int C, int H, int W,
                 int k, float loss_weight, int mean, float *loss_out, float *grad_output /* nullable */,
                 void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_local_variance(const float *residual, int B, int H, int W, int k, float *v_out /* nullable */,
                       const float *grad_v /* nullable */, float *grad_residual /* nullable */, void *workspace,
                       size_t workspace_bytes, ssg_stream_t stream);

/* ---------------------------------------------------------------- (G) ----
 * BebyGAN's best-buddy loss and flat mask (basicsr/models/bebyganssl_model.py:471-565 BBL.forward with its caller's
 * L1Loss(p1, sel_p2) at :723-724, and get_flat_mask at :93-104), ssl_amd/csrc/ssg_bbl.hip.  x, gt (B,C,H,W) fp32:
 *   p1 = unfold(x, k, stride), p2 = unfold(gt, k, stride)                        (B, N, d), d = C k^2
 *   cand = cat[p2, unfold(gt_2), unfold(gt_4)]                                   (B, M, d)
 *     gt_2, gt_4: bicubic 1/2 and 1/4 of gt (A = -0.75, align_corners = False, no antialias, side floor(side / 2 | / 4))
 *   ind_i = argmin_j alpha |p1_i - cand_j|^2 + beta |p2_i - cand_j|^2, evaluated in fp32 as
 *           (alpha + beta) |cand_j|^2 - 2 (alpha p1_i + beta p2_i) . cand_j; among equal fp32 scores the LOWEST j wins,
 *           so results are bit-reproducible
 *   sel_p2_i = cand[ind_i];  loss = loss_weight * mean |p1 - sel_p2| (mean != 0; the sum otherwise)
 *   grad_x = d loss / d x: loss_weight / (B N d) sgn(p1 - sel_p2) at each patch element's pixel, 0 at pixels outside the
 *           patch grid (every pixel is written); sgn(0) = 0.  gt carries no gradient.
 * Native domain: pad = 0, stride >= k >= 1, d <= 31, alpha, beta >= 0 with alpha + beta > 0.  Status: SSG_E_BADARG for a
 * null pointer (those marked nullable excepted), B, C, H, W or k <= 0, stride < k, a negative or NaN weight or
 * alpha + beta = 0; SSG_E_TOOLARGE for d > 31, B > 65535 or 2^31 elements and more; SSG_E_IMAGESMALL when gt_4 is
 * smaller than k on a side (H / 4 < k or W / 4 < k: the reference's unfold raises); SSG_E_WORKSPACE for workspace_bytes <
 * ssg_bbl_workspace_bytes(...) (which returns 0 for a shape outside the domain); SSG_E_ALIGN for a workspace that is
 * not 16-byte aligned.  Three launches (four with the loss), no atomics, no score matrix, fixed summation orders.
 * ssg_bbl_search: ind_out int32 (B,N); p1_out, sel_out (B,N,d), each nullable.
 * ssg_bbl_loss: loss_out[0]; grad_x (B,C,H,W) and ind_out (B,N), each nullable.
 * ssg_flat_mask: img (B,3,H,W); L = (0.2989 r + 0.587 g) + 0.114 b, reflect-padded by k / 2; mask_out (B,1,H,W) = 1.0
 *   where the unbiased standard deviation of the k x k window is < thresh, else 0.0.  k odd, 3 <= k <= 15 (11 is the
 *   compiled fast path).  SSG_E_BADARG for a null pointer, k even or < 3, B, H or W <= 0; SSG_E_TOOLARGE for k > 15;
 *   SSG_E_IMAGESMALL for H or W <= k / 2 (torch's reflect pad raises).  One launch. */
size_t ssg_bbl_workspace_bytes(int B, int C, int H, int W, int k, int stride);
int ssg_bbl_search(const float *x, const float *gt, int B, int C, int H, int W, int k, int stride, float alpha,
                   float beta, int *ind_out, float *p1_out /* nullable */, float *sel_out /* nullable */,
                   void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_bbl_loss(const float *x, const float *gt, int B, int C, int H, int W, int k, int stride, float alpha,
                 float beta, float loss_weight, int mean, float *loss_out, float *grad_x /* nullable */,
                 int *ind_out /* nullable */, void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_flat_mask(const float *img, int B, int H, int W, int k, float thresh, float *mask_out, ssg_stream_t stream);

/* ---------------------------------------------------------------- (H) ----
 * BebyGAN's back-projection loss and the imresize under it (basicsr/models/bebyganssl_model.py:727-731:
 * l_pix_bp = L1Loss(imresize(output, scale = 1 / s), lq); imresize at :375-469 on its integer-factor path,
 * discrete_kernel -> downsampling_2d, :133-162 and :351-373), ssl_amd/csrc/ssg_bp.hip.  x (planes,H,W) fp32 planes
 * (planes = B C); s the integer factor, 2, 3 or 4; K = 4s (s even) or 4s - 1 (s odd); p = (K - s) / 2:
 *   taps  w_i = c(r_i) / sum_j c(r_j), r_i = (i - (K-1)/2) / s, c the Keys cubic with a = -0.5 (MATLAB's antialiased
 *         bicubic), formed in fp64 and rounded once to fp32; the 2-D tap is w_i w_j
 *   pad   symmetric, p pixels per side: index -1-i reads pixel i, n+i reads n-1-i (the edge pixel is used twice)
 *   y[oy,ox] = sum_{i,j<K} w_i w_j x~[s oy + i - p, s ox + j - p], (planes,h,w) with h = H / s, w = W / s (floor)
 *   loss  = loss_weight * mean |y - lq| over the planes h w elements (mean != 0; the sum otherwise)
 *   grad_x = d loss / d x = loss_weight / M K^T sgn(y - lq), K^T the exact adjoint of the padding and the strided
 *         correlation (a pixel under one or both mirrors collects each of its padded copies); sgn(0) = 0; every pixel
 *         is written.  lq carries no gradient.
 * Status, decided before any launch: SSG_E_BADARG for a null pointer (those marked nullable excepted), planes, H or
 * W <= 0, s < 2 or a NaN loss_weight; SSG_E_TOOLARGE for s > 4 or 2^31 elements and more; SSG_E_IMAGESMALL for H or
 * W < p (the reference's padding loop raises); SSG_E_WORKSPACE for workspace_bytes < ssg_bp_workspace_bytes(...)
 * (which returns 0 for a shape outside the domain; it holds the signs and at most 4,096 partial sums: at most
 * 2 planes h w 4 bytes + 64 KiB, nothing of input size); SSG_E_ALIGN for a workspace that is not 16-byte aligned.
 * No atomics, fixed summation orders (bit-reproducible), no allocation, synchronisation or host read.
 * ssg_bp_downsample: y_out (planes,h,w); one launch.
 * ssg_bp_downsample_backward: grad_x (planes,H,W) = K^T grad_y (overwritten); one launch.
 * ssg_bp_loss: loss_out[0]; grad_x (planes,H,W) and y_out (planes,h,w), each nullable; two launches. */
size_t ssg_bp_workspace_bytes(int planes, int H, int W, int s);
int ssg_bp_downsample(const float *x, int planes, int H, int W, int s, float *y_out, ssg_stream_t stream);
int ssg_bp_downsample_backward(const float *grad_y, int planes, int H, int W, int s, float *grad_x,
                               ssg_stream_t stream);
int ssg_bp_loss(const float *x, const float *lq, int planes, int H, int W, int s, float loss_weight, int mean,
                float *loss_out, float *grad_x /* nullable */, float *y_out /* nullable */, void *workspace,
                size_t workspace_bytes, ssg_stream_t stream);

/* ---------------------------------------------------------------- (I) ----
 * The kernels the degradation chain convolves with (the dataset's per-sample kernel synthesis,
 * basicsr/data/my_realesrgan_image_mask_dataset.py:88-141 through basicsr/data/degradations.py:16-173,389-409),
 * ssl_amd/csrc/ssg_kernels.hip.  One record describes one K x K kernel, K = size:
 *   SSG_KERNEL_PULSE        1 at the centre, 0 elsewhere (the dataset's pulse_tensor)
 *   SSG_KERNEL_SINC         circular_lowpass_kernel: omega_c J1(omega_c r) / (2 pi r), r the distance from
 *                           ((K-1)/2, (K-1)/2); omega_c^2 / (4 pi) at the centre
 *   SSG_KERNEL_GAUSSIAN     bivariate_Gaussian: exp(-q / 2)
 *   SSG_KERNEL_GENERALIZED  bivariate_generalized_Gaussian: exp(-q^beta / 2)
 *   SSG_KERNEL_PLATEAU      bivariate_plateau: 1 / (q^beta + 1)
 * with q = g^T Sigma^-1 g on the grid g = (x, y), x, y in -(K/2) .. K/2, x along columns (mesh_grid), Sigma =
 * U diag(sig_x^2, sig_y^2) U^T, U the rotation by theta (sigma_matrix2; an isotropic kernel is sig_y = sig_x, theta =
 * 0).  Every kind but the pulse is divided by the sum of its K^2 values; the kernel then sits centred in a pad_to x
 * pad_to square of zeros at offset (pad_to - K) / 2 (the dataset's np.pad).  All arithmetic is fp64, Sigma's inverse
 * and the sum included; the one fp32 rounding is the store, so an element differs from the reference's
 * torch.FloatTensor(kernel) by one fp32 ulp at most.  Fields a kind does not use are ignored.
 *
 * ssg_synth_kernels: `records` are n records in HOST memory; they are checked, copied to `records_dev` (n records of
 * device memory, scratch) by one asynchronous copy on `stream` and expanded by one launch into out (n, pad_to, pad_to)
 * fp32, of which every element is written, the zeros included (out needs no clearing).  One workgroup per kernel, a
 * fixed-order sum, no atomics: bit-reproducible.  `records` may be released when the call has returned if it is
 * pageable memory (the runtime has staged it by then), and once the copy has completed on `stream` if it is pinned.
 * Status, decided before the copy and the launch: SSG_E_BADARG for n < 0, pad_to even, < 1 or > 21, a null pointer, a
 * record whose size is even, < 1 or > pad_to, or an unknown kind; n == 0 succeeds and does nothing. */
#define SSG_KERNEL_PULSE 0
#define SSG_KERNEL_SINC 1
#define SSG_KERNEL_GAUSSIAN 2
#define SSG_KERNEL_GENERALIZED 3
#define SSG_KERNEL_PLATEAU 4
typedef struct ssg_kernel_record {
  int32_t kind;   /* SSG_KERNEL_* */
  int32_t size;   /* K, odd, <= pad_to */
  double sig_x, sig_y, theta, beta, omega_c;
} ssg_kernel_record;   /* 48 bytes */
int ssg_synth_kernels(const ssg_kernel_record *records, int n, int pad_to, ssg_kernel_record *records_dev, float *out,
                      ssg_stream_t stream);

/* ---------------------------------------------------------------- (J) ----
 * The validation metrics (basicsr/metrics/psnr_ssim.py: calculate_psnr, calculate_ssim on what tensor2img,
 * basicsr/utils/img_util.py:37-93, hands them; to_y_channel and bgr2ycbcr in between), ssl_amd/csrc/ssg_metrics.hip.
 * Two images of one shape come in, one row of results per image goes out; nothing is copied to the host.
 *   kind      SSG_METRIC_F32_RGB  fp32 planar (B,C,H,W), RGB, nominal [0, 1] (a model's tensors): quantised as
 *                                 q = rint(fl32(clamp(x, 0, 1) * 255.0f)), ties to even, and read in BGR order
 *             SSG_METRIC_U8_HWC   uint8 interleaved (B,H,W,C), BGR (a decoded image file)
 *             SSG_METRIC_U8_CHW   uint8 planar (B,C,H,W), BGR
 *   crop      crop_border pixels from each side; 0 = none
 *   planes    y_channel != 0, C = 3: v_c = fl32(q_c / 255.0f); t = ((24.966 v_b + 128.553 v_g) + 65.481 v_r) + 16.0
 *             in fp64 without fma; the one plane is fl32(fl32(t / 255.0) * 255.0f).  y_channel != 0, C = 1:
 *             fl32(fl32(q / 255.0f) * 255.0f).  y_channel == 0: the C planes are the integers q, in BGR order.
 *   PSNR      10 log10(255^2 / mse), mse the fp64 mean of the squared plane differences over planes and pixels (summed
 *             in integers, exactly, when y_channel == 0); +inf where mse == 0
 *   SSIM      per plane the five moments under the 11 x 11 Gaussian window (sigma 1.5) on the 'valid' region
 *             (H - 2 crop - 10) x (W - 2 crop - 10), c1 = (0.01 * 255)^2, c2 = (0.03 * 255)^2, the map
 *             ((2 mu1 mu2 + c1)(2 s12 + c2)) / ((mu1^2 + mu2^2 + c1)(s1 + s2 + c2)), its mean over map and planes; fp64
 * A NaN in a float input is unspecified (the reference's uint8 cast of NaN is undefined).
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer, B, H or W <= 0, C not
 * 1 or 3, crop_border < 0 or an unknown kind; SSG_E_TOOLARGE for B > 65535 or 2^31 elements and more;
 * SSG_E_IMAGESMALL for a cropped side shorter than 11 (the reference would return the mean of an empty map; for the
 * planes alone: shorter than 1); SSG_E_WORKSPACE for workspace_bytes < the size reported for the shape (which is 0 for
 * a shape outside the domain; it holds at most 512 partial sums of three kinds per image: 12 KiB per image + 768 bytes
 * at most, nothing of image size); SSG_E_ALIGN for a workspace that is not 16-byte aligned.
 * No atomics, fixed summation orders (bit-reproducible), no allocation, synchronisation or host read.
 * ssg_psnr_ssim: out (B,4) fp64 on the device: PSNR, SSIM, the sum of the squared plane differences, the number of
 *   values in that sum.  Two launches.
 * ssg_metric_planes: planes_out (B,P,H - 2 crop,W - 2 crop) fp32, P = 1 with y_channel and C otherwise: the planes
 *   the metrics are computed on.  One launch. */
#define SSG_METRIC_F32_RGB 0
#define SSG_METRIC_U8_HWC 1
#define SSG_METRIC_U8_CHW 2
size_t ssg_metric_workspace_bytes(int B, int C, int H, int W, int crop_border);
int ssg_psnr_ssim(const void *a, const void *b, int kind, int B, int C, int H, int W, int crop_border, int y_channel,
                  double *out, void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_metric_planes(const void *img, int kind, int B, int C, int H, int W, int crop_border, int y_channel,
                      float *planes_out, ssg_stream_t stream);

/* ---------------------------------------------------------------- (K) ----
 * NIQE (basicsr/metrics/niqe.py: calculate_niqe, niqe, compute_feature, estimate_aggd_param; to_y_channel and the 1/2
 * imresize of basicsr/utils/matlab_functions.py in between), ssl_amd/csrc/ssg_niqe.hip.  One image in, one score per
 * image out; nothing is copied to the host.  Computed in fp64 from the integer plane on (the reference keeps fp32 by
 * accident of an astype; MATLAB's original is double): the contract, stage by stage, heads ssg_niqe.hip.
 *   kind      the three SSG_METRIC_* kinds of section (J), read the same way, and
 *             SSG_NIQE_F32_PLANE  fp32 (B,H,W) (C = 1): input_order 'HW', the given plane; `convert` is not looked at
 *   convert   0 'y': to_y_channel as in section (J) (C = 1: the grey round trip); 1 'gray' (C = 3 only): OpenCV's
 *             DOCUMENTED BGR2GRAY, 0.114 B + 0.587 G + 0.299 R on q / 255 in fp32, then * 255 -- OpenCV was never run
 *             against it, its documentation alone pins the formula
 *   plane 1   the converted plane, crop_border pixels off every side, rounded half to even, then its top-left
 *             96 nbh x 96 nbw, nbh = (H - 2 crop) / 96, nbw = (W - 2 crop) / 96; plane 2 (48 nbh x 48 nbw) is its
 *             antialiased bicubic half (not rounded).  Blocks are 96 x 96 and 48 x 48, nblk = nbh nbw per image.
 *   features  (B, nblk, 36) fp64: 18 per scale, the reference's order; rows in its block order (block column outer).
 *             A block side without a negative or without a positive value gives NaN entries (and alpha = 0.2, np.argmin's
 *             answer to NaN), as in the reference.
 *   score     sqrt(d' S^-1 d), S = (cov_pris + cov) / 2, by Cholesky (= the reference's pinv wherever S is finite);
 *             NaN for fewer than two NaN-free rows.  mu_pris (36), cov_pris (36,36) fp64 on the device.
 * A NaN in a float input is unspecified.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer, B, H or W <= 0, C not
 * 1 or 3 (the plane kind: not 1), crop_border < 0, an unknown kind, convert not 0 or 1, or 'gray' with C = 1;
 * SSG_E_TOOLARGE for B > 65535 or 2^31 elements and more; SSG_E_IMAGESMALL for a cropped side shorter than 96 (no
 * block); SSG_E_WORKSPACE for workspace_bytes < ssg_niqe_workspace_bytes(...) (0 for a shape outside the domain; it
 * holds both planes, the features and one flag per row: about 6.2 bytes per pixel of plane 1); SSG_E_ALIGN for a
 * workspace that is not 16-byte aligned.
 * No atomics, fixed summation orders (bit-reproducible), no synchronisation or host read.  The first call per device
 * of ssg_niqe / ssg_niqe_features uploads the 306 KiB table of the alpha search (one allocation, one blocking copy):
 * make it outside stream capture.
 * ssg_niqe: out (B) fp64 on the device.  Five launches.
 * ssg_niqe_planes: plane1 (B,96 nbh,96 nbw) fp32, plane2 (B,48 nbh,48 nbw) fp64.  Two launches.
 * ssg_niqe_features: feat (B,nblk,36) fp64; the planes go to the workspace.  Three launches.
 * ssg_niqe_table: HOST function, no device: table_out (4,9801) fp64 = gam, r(gam) = G(2/g)^2 / (G(1/g) G(3/g)),
 *   G(1/g) / G(3/g), G(2/g) / G(1/g) -- what the device's table holds. */
#define SSG_NIQE_F32_PLANE 3
size_t ssg_niqe_workspace_bytes(int B, int C, int H, int W, int crop_border);
int ssg_niqe(const void *img, int kind, int B, int C, int H, int W, int crop_border, int convert, const double *mu_pris,
             const double *cov_pris, double *out, void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_niqe_planes(const void *img, int kind, int B, int C, int H, int W, int crop_border, int convert, float *plane1,
                    double *plane2, ssg_stream_t stream);
int ssg_niqe_features(const void *img, int kind, int B, int C, int H, int W, int crop_border, int convert, double *feat,
                      void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_niqe_table(double *table_out);

/* ---------------------------------------------------------------- (L) ----
 * StableSR's colour correction of the Diffusion fork's samples (scripts/wavelet_color_fix.py: wavelet_blur,
 * wavelet_decomposition, wavelet_reconstruction, calc_mean_std, adaptive_instance_normalization, and the
 * clamp((x + 1) / 2, 0, 1) and 255 x -> byte its callers append), ssl_amd/csrc/ssg_colorfix.hip.  Every tensor fp32
 * contiguous (B,C,H,W), any B, C, H, W >= 1, planes independent; content first, style second, as in the reference.
 *   blur      [1/4, 1/2, 1/4] per axis at -radius, 0, +radius, the tap coordinate clamped to the plane (replicate
 *             padding by `radius`, then the dilated 3 x 3 convolution); rows first, then columns.
 *   levels    1 .. 5 (5: the reference's default and only use): level i has radius 2^(i-1); low = the image after all
 *             levels, high = image - low (the reference sums the per-level differences, which telescope to this).
 *   wavelet   out = content + low(style - content), which is high(content) + low(style) in real arithmetic: the blur
 *             is linear and clamps both images alike.  Within 64 * 2^-24 * max(|content|, |style|) of the fp64 value.
 *   stats     per plane {mean, sqrt(var + eps)}, var unbiased (n - 1; a plane of one element gives NaN, as torch), fp64
 *             sums in a fixed order over a fixed chunking: the same bits whatever the batch around the plane.
 *             stats (n_img, B C, 2) fp64 on the device, image 0 = content, image 1 = style (n_img = 1 for a null style).
 *   adain     out = (x - mean_c) / std_c * std_s + mean_s on the statistics rounded to fp32; stats (2, B C, 2) as
 *             ssg_colorfix_stats wrote it, or NULL: the epilogue alone ('nofix').
 *   out_kind  SSG_COLORFIX_RAW v, fp32 (B,C,H,W); SSG_COLORFIX_UNIT u = clamp((v + 1) / 2, 0, 1), fp32 (B,C,H,W), a NaN
 *             stays a NaN; SSG_COLORFIX_U8_NHWC (uint8)(255.0f u) truncated, uint8 (B,H,W,C), a NaN gives 0.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer (those marked nullable
 * excepted: `style` of ssg_colorfix_stats, `stats` of ssg_colorfix_adain, one of high / low), an output that is an input
 * (ssg_colorfix_adain may run in place for the two fp32 kinds), B, C, H or W <= 0, radius < 1, levels < 1, an unknown
 * out_kind, eps < 0 or NaN; SSG_E_TOOLARGE for levels > 5 or 2^31 elements and more; SSG_E_WORKSPACE for
 * workspace_bytes < ssg_colorfix_workspace_bytes(...) (0 for a shape outside the domain; 48 bytes per 4,096 elements of a
 * plane: the chunk sums of both images); SSG_E_ALIGN for a workspace that is not 16-byte aligned.
 * No atomics, no synchronisation, no allocation, no host read; bit-reproducible.
 * ssg_wavelet_blur: one launch, taps read from global memory, any radius >= 1.
 * ssg_wavelet_decompose: high, low (B,C,H,W), either may be NULL.  One launch (64 x 64 tiles, 128,016 B of LDS).
 * ssg_colorfix_wavelet: one launch of the same tile pass.
 * ssg_colorfix_stats: two launches for one image or two.   ssg_colorfix_adain: one launch. */
#define SSG_COLORFIX_RAW 0
#define SSG_COLORFIX_UNIT 1
#define SSG_COLORFIX_U8_NHWC 2
int ssg_wavelet_blur(const float *image, int B, int C, int H, int W, int radius, float *out, ssg_stream_t stream);
int ssg_wavelet_decompose(const float *image, int B, int C, int H, int W, int levels, float *high, float *low,
                          ssg_stream_t stream);
int ssg_colorfix_wavelet(const float *content, const float *style, int B, int C, int H, int W, int levels, int out_kind,
                         void *out, ssg_stream_t stream);
size_t ssg_colorfix_workspace_bytes(int B, int C, int H, int W);
int ssg_colorfix_stats(const float *content, const float *style, int B, int C, int H, int W, double eps, double *stats,
                       void *workspace, size_t workspace_bytes, ssg_stream_t stream);
int ssg_colorfix_adain(const float *content, const double *stats, int B, int C, int H, int W, int out_kind, void *out,
                       ssg_stream_t stream);

/* ---------------------------------------------------------------- (M) ----
 * KAIR's SSIM criterion (GAN-Based-SR/train_BSGRAN/models/loss_ssim.py: _ssim, SSIMLoss, ssim -- the pytorch-ssim
 * module, G_lossfn_type "ssim" of models/model_ssl.py), ssl_amd/csrc/ssg_ssim.hip.  x, y fp32 contiguous (B,C,H,W), any
 * B, C, H, W >= 1 (sides shorter than the window included), planes independent; everything is computed in fp32 but
 * the sums.  With `*` the per-plane 'same' convolution (zero padding) under the window w_ij = g_i g_j, g the
 * window_size normalised Gaussian taps of sigma 1.5 in fp32:
 *   mx = w*x, my = w*y, exx = w*x^2, eyy = w*y^2, exy = w*xy
 *   A1 = 2 mx my + C1, A2 = 2 (exy - mx my) + C2, B1 = mx^2 + my^2 + C1, B2 = (exx - mx^2) + (eyy - my^2) + C2,
 *   C1 = 0.01^2, C2 = 0.03^2, S = A1 A2 / (B1 B2)
 *   sums_out[b] = the sum of S over image b, b < B; sums_out[B] = their sum in image order: B + 1 DOUBLES on the
 *         device (the map values are fp32, their accumulation is fp64).  SSIM is sums_out[B] / (B C H W), or
 *         sums_out[b] / (C H W) per image; sign and weight are the caller's.
 *   grad_x (nullable) = d sums_out[B] / d x = w*P + 2 x (w*Q) + y (w*R), P = dS/dmx (through both variances), Q =
 *         -S / B2, R = 2 A1 / (B1 B2), each zero outside the image; every element is written.  UNSCALED: multiply by
 *         the upstream coefficient of S (1 / (B C H W) for the mean).  S is symmetric, so the gradient with respect to
 *         y is the call with x and y exchanged.  With a null grad_x the tile pass skips the ring and the store.
 * window_size is odd and <= 11; a smaller window is the 11-tap kernel with zero taps beyond its radius.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer (grad_x excepted), a
 * grad_x that is x or y, B, C, H or W <= 0, or a window_size that is even, < 1 or > 11; SSG_E_TOOLARGE for B > 65535 or
 * 2^31 elements and more; SSG_E_WORKSPACE for workspace_bytes < ssg_ssim_workspace_bytes(...) (0 for a shape outside
 * the domain; one double per workgroup: min(C ceil(H / 32) ceil(W / 64), ssg_ssim_grid_cap()) per image, padded to
 * 256 bytes); SSG_E_ALIGN for a workspace that is not 16-byte aligned.
 * Two launches.  No atomics, fixed summation orders: bit-reproducible, and image b of a batch gets the bits it gets
 * alone.  No allocation, synchronisation or host read.
 * ssg_ssim_grid_cap: the most workgroups per image the tile pass launches (512); beyond it a workgroup walks several
 *   tiles.
 * ssg_ssim_taps: HOST function, no device: taps_out[11] = the fp32 taps the kernels use, centred, zeros around a
 *   window shorter than 11 (the reference's gaussian(window_size, 1.5)). */
size_t ssg_ssim_workspace_bytes(int B, int C, int H, int W);
int ssg_ssim_grid_cap(void);
int ssg_ssim_taps(int window_size, float *taps_out);
int ssg_ssim_loss(const float *x, const float *y, int B, int C, int H, int W, int window_size,
                  float *grad_x /* nullable */, double *sums_out, void *workspace, size_t workspace_bytes,
                  ssg_stream_t stream);

/* ---------------------------------------------------------------- (N) ----
 * Pillow's 8-bit convolution resize (PIL.Image.resize(size, resample) with box=None, reducing_gap=None: libImaging's
 * ImagingResample) -- the LANCZOS resize of the Diffusion fork's load_img (test.py:111-120) and of the multiscale
 * preparation scripts (generate_multiscale_img.py, generate_multiscale_DF2K.py), ssl_amd/csrc/ssg_resample.hip.  The
 * algorithm is integer from its coefficient tables on, so the bytes are Pillow's: no tolerance.
 * For one axis with input size `in` and output size `out`, S = 3 (LANCZOS), 2 (BICUBIC), 1 (BILINEAR, HAMMING), 0.5 (BOX):
 *   scale = in / out, fs = max(scale, 1), support = S fs, ksize = 2 ceil(support) + 1; for every output index xx
 *   center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), in)
 *   - xmin, w_i = f((i + xmin - center + 0.5) (1 / fs)), ww their sum in index order, w_i /= ww when ww != 0, all fp64;
 *   k_i = (int)(w_i 2^22 + 0.5) for w_i >= 0, (int)(w_i 2^22 - 0.5) otherwise (C truncation); zeros from n to ksize.
 *   A pass is clip8((2^21 + sum_i px[xmin + i] k_i) >> 22) on an int32 accumulator.  The columns are filtered first, into
 *   bytes; the rows are filtered from those bytes.  A pass whose axis keeps its size is not run; bands are independent.
 * ssg_resample_ksize, ssg_resample_table: HOST functions, no device: the tables above, with the C library's sin and cos
 *   (computing them on the device could move a coefficient by one).  bounds[out][2] = {xmin, n}, coef[out][ksize].
 *   ksize < 0 is a status (SSG_E_BADARG for in, out < 1 or an unknown filter).
 * ssg_resample: src uint8 (B,Hin,Win,C) contiguous on the device, C 1 or 3; the four tables int32 on the device, those of
 *   an axis that keeps its size are not read and may be NULL.  One launch: a workgroup of 256 threads per output tile
 *   reads the tile's input footprint into LDS, filters its columns into a byte intermediate in LDS and the rows from
 *   that.  No atomics: image b of a batch gets the bytes it gets alone.  No allocation, synchronisation or host read.
 *   out_kind  SSG_RESAMPLE_U8_HWC the byte v, uint8 (B,Hout,Wout,C); SSG_RESAMPLE_F32_UNIT (float)v / 255.0f, fp32
 *             (B,C,Hout,Wout) (what ssg_edge_mask_laplacian takes); SSG_RESAMPLE_F32_SIGNED 2.0f ((float)v / 255.0f) -
 *             1.0f, fp32 (B,C,Hout,Wout): load_img's numpy / torch expression bit for bit.
 *   The tile is chosen per call from a short list (32 x 64, 16 x 64, 16 x 32, 8 x 32): the first whose footprint,
 *   intermediate and coefficient rows take at most 20 KiB of LDS (eight workgroups per CU), else the one that takes the
 *   least, which must fit the 160 KiB of a CU.  The fused kernel takes every ratio in / out <= 8 per axis for all five
 *   filters (114,176 B at most); beyond that ssg_resample returns SSG_E_TOOLARGE (resize in two steps, or on the CPU).
 * Status, decided before the launch with the output untouched: SSG_E_BADARG for a null src or out, out == src, a null
 * table of an axis that changes size, C not 1 or 3, B or a size < 1, an unknown filter or out_kind; SSG_E_TOOLARGE for
 * more than 2^31 - 1 input or output elements, or in > 8 out on an axis.
 * ssg_resample_tile: the first tile of the list (rows, columns); every other tile divides it.
 * ssg_resample_max_ratio: 8. */
#define SSG_RESAMPLE_LANCZOS 1   /* Pillow's Image.Resampling numbers */
#define SSG_RESAMPLE_BILINEAR 2
#define SSG_RESAMPLE_BICUBIC 3
#define SSG_RESAMPLE_BOX 4
#define SSG_RESAMPLE_HAMMING 5
#define SSG_RESAMPLE_U8_HWC 0
#define SSG_RESAMPLE_F32_UNIT 1
#define SSG_RESAMPLE_F32_SIGNED 2
int ssg_resample_ksize(int in, int out, int filter);
int ssg_resample_table(int in, int out, int filter, int *bounds, int *coef);
int ssg_resample_tile(int *tile_rows, int *tile_cols);
int ssg_resample_max_ratio(void);
int ssg_resample(const uint8_t *src, int B, int C, int Hin, int Win, int Hout, int Wout, int filter, const int *xbounds,
                 const int *xcoef, const int *ybounds, const int *ycoef, int out_kind, void *out, ssg_stream_t stream);

/* ---------------------------------------------------------------- (O) ----
 * MATLAB's bicubic imresize as the reference's Python restates it (basicsr/utils/matlab_functions.py:imresize, KAIR's
 * utils_image.py:imresize / imresize_np; generate_bicubic_img.m calls the original), ssl_amd/csrc/ssg_imresize.hip: any
 * scale > 0 (the same on both axes), with or without antialiasing, evaluated in fp64.
 * For one axis with input length n and scale s:
 *   m = ceil(n s) in doubles; kw = 4 / s when s < 1 and antialias != 0, else 4; T = ceil(kw) taps per output.
 *   For output k = 1 .. m (1-based): u = k / s + 0.5 (1 - 1 / s), left = floor(u - kw / 2), taps j = left + 1 .. left + T,
 *   v_j = s c(s (u - j)) under antialiasing, c(u - j) otherwise, c Keys' cubic with a = -0.5 in the order of operations
 *   written out in ssg_imresize.hip; w_j = v_j / (the sum of the v_j in index order).  All fp64, no fused multiply-add.
 *   A tap outside the image is mirrored symmetrically ON THE INDEX: 0-based j < 0 reads -1 - j, j >= n reads 2 n - 1 - j.
 *   Every tap must reach the image with one reflection, -n <= j <= 2 n - 1 (the reference's padding copy raises
 *   outside that): such an axis is refused with SSG_E_IMAGESMALL.
 *   The columns are filtered first, into fp64; the rows are filtered from that: fp64 sums in tap order from 0.0.
 * ssg_imresize_out_size: m, or SSG_E_BADARG (n < 1, scale <= 0, not finite, or n s = 0) / SSG_E_TOOLARGE (m >= 2^31).
 * ssg_imresize_taps: T, or SSG_E_BADARG (scale) / SSG_E_TOOLARGE (T > 32: antialiased scales below 1 / 8).
 * ssg_imresize_table: HOST function, no device.  first[m] = left (the first tap's 0-based index, before the mirror),
 *   weights[m][T].  m must be ssg_imresize_out_size(n, scale) (SSG_E_BADARG otherwise); the statuses of the two
 *   functions above, and SSG_E_IMAGESMALL for the mirror domain, with both arrays untouched.
 * ssg_imresize_tiles: writes the (rows, columns) of up to `capacity` tiles of the kernel's list, returns how many the
 *   list has, and with `chosen` non-null the index of the tile a call at (scale, antialias) takes (-1: invalid scale, too
 *   many taps).
 * ssg_imresize: one launch for B C planes.  in_kind SSG_IMRESIZE_IN_F32: src fp32 (B,C,Hin,Win), any C >= 1, out_kind
 *   SSG_IMRESIZE_F32_PLANES: (float)y, fp32 (B,C,Hout,Wout), rounded once.  in_kind SSG_IMRESIZE_IN_U8_HWC: src uint8
 *   (B,Hin,Win,C), C 1 or 3, y summed over the byte values 0 .. 255 themselves; out_kind SSG_IMRESIZE_U8_HWC the byte
 *   v = min(255, floor(y + 0.5)) for y >= 0 and 0 below (MATLAB's round-half-away on uint8), uint8 (B,Hout,Wout,C), or
 *   SSG_IMRESIZE_F32_UNIT (float)v / 255.0f, fp32 (B,C,Hout,Wout) (what ssg_edge_mask_laplacian takes).  The four
 *   tables are those of ssg_imresize_table for (Hin, Hout) and (Win, Wout), on the device.  A workgroup of 256 threads
 *   per output tile and plane reads the tile's mirrored footprint into LDS as fp32, filters the columns into an fp64
 *   intermediate in LDS and the rows from that.  No atomics: plane b of a batch gets the bits it gets alone, and a
 *   repeat gives the same bits.  No allocation, synchronisation or host read.
 * Status, decided before the launch with the output untouched: SSG_E_BADARG for a null pointer, out == src, B, C or a
 * size < 1, C not 1 or 3 for bytes, an unknown kind or a pair of kinds not listed above, a scale <= 0 or not finite;
 * SSG_E_TOOLARGE for more than 32 taps or 2^31 input or output elements and more; SSG_E_IMAGESMALL for a side outside
 * the mirror domain.  Every upscale and every non-antialiased scale has four taps and is in the domain: where the taps
 * of neighbouring outputs lie further apart than they are wide, the footprint holds four entries per output. */
#define SSG_IMRESIZE_IN_F32 0
#define SSG_IMRESIZE_IN_U8_HWC 1
#define SSG_IMRESIZE_F32_PLANES 0
#define SSG_IMRESIZE_U8_HWC 1
#define SSG_IMRESIZE_F32_UNIT 2
int ssg_imresize_out_size(int n, double scale);
int ssg_imresize_taps(double scale, int antialias);
int ssg_imresize_table(int n, int m, double scale, int antialias, int *first, double *weights);
int ssg_imresize_tiles(double scale, int antialias, int *tiles, int capacity, int *chosen /* nullable */);
int ssg_imresize(const void *src, int in_kind, int B, int C, int Hin, int Win, double scale, int antialias,
                 const int *yfirst, const double *yweights, const int *xfirst, const double *xweights, int out_kind,
                 void *out, ssg_stream_t stream);

/* ---------------------------------------------------------------- (P) ----
 * libjpeg's baseline JPEG round trip, encode at a quality and decode again, without the bitstream: what the reference
 * reaches through cv2.imencode / cv2.imdecode (KAIR's utils_blindsr.py:412-418 add_JPEG_noise, basicsr's
 * degradations.py add_jpg_compression, scripts/util_image.py:366-383 jpeg_compress), ssl_amd/csrc/ssg_jpegcodec.hip.
 * jpeg_set_quality(quality, force_baseline), 4:2:0 for colour, the "islow" integer DCT pair, fancy upsampling, no
 * smoothing: the eight integer stages written out at the top of ssg_jpegcodec.hip and restated in
 * tests/jpeg_codec_reference.py, to which the result is EQUAL, byte for byte, for every H, W >= 1.
 * ssg_jpeg_roundtrip: `in` SSG_JPEG_IN_U8_HWC uint8 (B,H,W,channels), or SSG_JPEG_IN_F32_NCHW fp32 (B,channels,H,W)
 *   quantised as rint(min(max(x, 0), 1) 255.0f) (round half to even); channels 1 (grey) or 3 (RGB).  `qualities`: B ints
 *   1 .. 100 on the HOST, read before the call returns (they travel as kernel arguments, 256 images a launch).  `out`
 *   SSG_JPEG_OUT_U8_HWC the bytes, uint8 (B,H,W,channels), or SSG_JPEG_OUT_F32_NCHW fp32 (B,channels,H,W) holding
 *   (float)((double)v / 255.0), the 256 values ssg_jpeg_unit_table writes (numpy's float32(v / 255.)).
 *   A workgroup of 256 threads codes a tile of 32 x 32 pixels in LDS.  The chroma upsampling reads one sample beyond the
 *   tile, so a colour call writes the reconstructed Y, Cb and Cr bytes to `workspace` and upsamples and converts in a
 *   second launch (measured against one launch that recomputes the chroma blocks around each tile:
 *   profiles/jpeg_codec_tile_ab.txt); a grey call is one launch and takes no workspace (`workspace` may be NULL).
 *   ssg_jpeg_roundtrip_workspace_bytes: B (H W + 2 ceil(H / 2) ceil(W / 2)) bytes with each image's share rounded up to
 *   256 for channels = 3, 0 for channels = 1 (and for arguments the call would refuse).
 *   No atomics: image b of a batch gets the bytes it gets alone, and a repeat gives the same bytes.  No allocation,
 *   synchronisation or device read of host memory.
 * Status, decided before the launch with the output untouched: SSG_E_BADARG for a null in, out or qualities, out == in,
 * a null workspace where one is needed, B or a size < 1, channels not 1 or 3, an unknown layout or epilogue, a quality
 * outside 1 .. 100; SSG_E_TOOLARGE for 2^31 elements or more; SSG_E_WORKSPACE for a workspace smaller than
 * ssg_jpeg_roundtrip_workspace_bytes(); SSG_E_ALIGN for one that is not 16-byte aligned. */
#define SSG_JPEG_IN_U8_HWC 0
#define SSG_JPEG_IN_F32_NCHW 1
#define SSG_JPEG_OUT_U8_HWC 0
#define SSG_JPEG_OUT_F32_NCHW 1
size_t ssg_jpeg_roundtrip_workspace_bytes(int B, int H, int W, int channels);
int ssg_jpeg_unit_table(float *table /* 256 floats, host */);
int ssg_jpeg_roundtrip(const void *in, void *out, int B, int H, int W, int channels, const int *qualities,
                       int in_layout, int out_epilogue, void *workspace, size_t workspace_bytes, ssg_stream_t stream);

/* ---------------------------------------------------------------- (Q) ----
 * The GAN criteria, plain and relativistic (basicsr/losses/gan_loss.py:11-140 GANLoss / MultiScaleGANLoss; KAIR's
 * train_BSGRAN/models/loss.py:135-172 GANLoss; the relativistic-average lines cri_gan(real - torch.mean(fake), ...) of
 * the nine basicsr/models/ *ssl_model.py files and of KAIR's model_ssl.py), ssl_amd/csrc/ssg_gan.hip.  x fp32, n >= 1
 * elements; the criteria are means over every element, so no shape is taken.  Per element d = x - shift[0] in fp32 with
 * one rounding (shift: one float ON THE DEVICE, the mean of the other tensor of a relativistic call; NULL: d = x), and
 * with t = label, s = sign (+1 or -1; it is checked for every kind and used by the last three):
 *   SSG_GAN_BCE       l = max(d, 0) - d t + log1p(exp(-|d|))      l' = sigmoid(d) - t      vanilla; KAIR gan, ragan
 *   SSG_GAN_LS        l = (d - t)^2                                l' = 2 (d - t)           lsgan
 *   SSG_GAN_LINEAR    l = s d                                      l' = s                   wgan, the hinge generator
 *                                                                                           term, plain sums (s = 1)
 *   SSG_GAN_SOFTPLUS  l = softplus(s d)                            l' = s sigmoid(s d)      wgan_softplus, softplusgan
 *   SSG_GAN_HINGE     l = relu(1 + s d)                            l' = s where 1 + s d > 0 (or NaN), else 0: exactly
 *                                                                       0 at 1 + s d = 0, as torch's ReLU gives it
 * Every operation is fp32, rounded once, in overflow-safe form (d = +-100 gives 100 or 0, never inf or NaN); a NaN
 * element is never dropped by a max: it reaches the sum.
 * ssg_gan_sums: sums_out[0] = sum of l(d_i), sums_out[1] = sum of l'(d_i): TWO DOUBLES on the device, the fp32 element
 *   values added in fp64 in a fixed order (one partial pair per workgroup in `workspace`, at most ssg_gan_grid_cap()
 *   workgroups of 256 threads and four elements per thread and trip, then one folding workgroup; a call of a single
 *   workgroup, n <= 1024, writes sums_out itself and is one launch).  No atomics: the same bits from call to call.  The
 *   mean of a tensor is SSG_GAN_LINEAR with s = 1 over n; sum l' is what the path through a relativistic mean needs.
 * ssg_gan_grad: grad[i] = (float)(coef[0] * l'(d_i) + coef[1]), coef TWO DOUBLES on the device: coef[0] carries
 *   upstream x weight / n, coef[1] the constant that flows back through a mean (0 without one).  One launch.
 * Loads and stores are 16 bytes wide behind a scalar head and in front of a scalar tail: x and grad need only a
 * float's own alignment.  No allocation, synchronisation or host read.
 * ssg_gan_workspace_bytes: 16 bytes per workgroup of the cap (16,384), whatever n.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer (shift excepted), n = 0,
 * a kind outside 0 .. 4 or a sign other than +1 or -1; SSG_E_ALIGN for an x or grad that is not 4-byte aligned or a
 * workspace, sums_out or coef that is not 8-byte aligned. */
#define SSG_GAN_BCE 0
#define SSG_GAN_LS 1
#define SSG_GAN_LINEAR 2
#define SSG_GAN_SOFTPLUS 3
#define SSG_GAN_HINGE 4
size_t ssg_gan_workspace_bytes(void);
int ssg_gan_grid_cap(void);
int ssg_gan_sums(const float *x, size_t n, int kind, float sign, float label, const float *shift /* nullable */,
                 void *workspace, double *sums_out, ssg_stream_t stream);
int ssg_gan_grad(const float *x, size_t n, int kind, float sign, float label, const float *shift /* nullable */,
                 const double *coef, float *grad, ssg_stream_t stream);

/* ---------------------------------------------------------------- (R) ----
 * SPSR's gradient map and the pixel criteria on it (basicsr/models/spsrssl_model.py:18-84 Get_gradient and
 * Get_gradient_nopadding, which are the same arithmetic; :363 cri_pix_gradSR(G(output), G(gt)); :368
 * cri_pix_gradBranch(branch, G(gt)); basicsr/losses/basic_loss.py:69-128 MSELoss, CharbonnierLoss),
 * ssl_amd/csrc/ssg_spsr.hip.  fp32 NCHW contiguous; a batch is planes = B C independent H x W planes, planes, H, W >= 1,
 * planes H W < 2^31.  Every operation is fp32 and rounded on its own (no fused multiply-add):
 *   map       v = x[i+1,j] - x[i-1,j], h = x[i,j+1] - x[i,j-1], a neighbour outside the plane is 0 (never read: with
 *             H = 1 or W = 1 that difference is 0), m = sqrtf((v v + h h) + 1e-6f).
 *   adjoint   dx[i,j] = ((a[i-1,j] - a[i+1,j]) + b[i,j-1]) - b[i,j+1], a = (w v) / m, b = (w h) / m recomputed from x
 *             at the neighbour (terms outside the plane are 0), w the gradient that arrives at the map value.
 *   criteria  d = p - q;  SSG_PIX_L1 |d|, l' = sign(d) with sign(0) = 0;  SSG_PIX_MSE d d, l' = 2 d;
 *             SSG_PIX_CHARBONNIER sqrtf(d d + eps), l' = d / sqrtf(d d + eps).  eps is read by the last only but is
 *             checked for every kind.
 * ssg_spsr_map: map = G(x).  One launch.
 * ssg_spsr_map_backward: grad_x = the adjoint with w = grad_map; x is all the state.  One launch.
 * ssg_spsr_loss: sum_out[0] = sum of crit(G(x) - G(target)), ONE DOUBLE on the device, neither map stored -- unless
 *   map_out is given, which receives G(x), the same bits as ssg_spsr_map's.  The fp32 element values are added in fp64 in
 *   a fixed order: one partial per workgroup in `workspace`, at most ssg_spsr_grid_cap() workgroups of 256 threads, four
 *   elements per thread and trip, then one folding workgroup (a call of a single workgroup, planes H W <= 1024, writes
 *   sum_out itself).  No atomics: the same bits from call to call.
 * ssg_spsr_loss_backward: grad_x = the adjoint with w = (float)(coef[0] crit'(m_x - m_target)) + grad_map: coef ONE
 *   DOUBLE on the device (upstream x weight / n), grad_map the nullable upstream gradient of the emitted map.  One
 *   launch serves the loss and whatever else consumed the map.  No gradient for the target.
 * ssg_spsr_branch_loss / _grad: sum_out[0] = sum of crit(branch - G(gt)) with G(gt) formed on the fly, and
 *   grad_branch[i] = (float)(coef[0] crit'(branch_i - G(gt)_i)); element-wise streams.
 * ssg_pixel_sums / _grad: the same two for two flat tensors of n >= 1 elements, sum of crit(pred - target) and
 *   (float)(coef[0] crit'(pred_i - target_i)): MSELoss and CharbonnierLoss (and L1).
 * Accesses are 16 bytes wide behind a scalar head and in front of a scalar tail wherever the tensors share the first
 * one's alignment; every tensor needs only a float's own alignment and W need not be a multiple of 4.  Plane p of a
 * batch is the same bits as the plane computed alone.  No allocation, synchronisation or host read.
 * ssg_spsr_workspace_bytes: 8 bytes per workgroup of the cap, whatever the shape.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer (map_out and grad_map
 * of the two loss calls excepted), planes, H, W or n < 1, planes H W >= 2^31, a kind outside 0 .. 2, an eps that is
 * negative or not finite; SSG_E_ALIGN for a float pointer that is not 4-byte aligned or a workspace, sum_out or coef
 * that is not 8-byte aligned. */
#define SSG_PIX_L1 0
#define SSG_PIX_MSE 1
#define SSG_PIX_CHARBONNIER 2
size_t ssg_spsr_workspace_bytes(void);
int ssg_spsr_grid_cap(void);
int ssg_spsr_map(const float *x, int planes, int H, int W, float *map, ssg_stream_t stream);
int ssg_spsr_map_backward(const float *x, const float *grad_map, int planes, int H, int W, float *grad_x,
                          ssg_stream_t stream);
int ssg_spsr_loss(const float *x, const float *target, int planes, int H, int W, int kind, float eps,
                  float *map_out /* nullable */, void *workspace, double *sum_out, ssg_stream_t stream);
int ssg_spsr_loss_backward(const float *x, const float *target, const float *grad_map /* nullable */, const double *coef,
                           int planes, int H, int W, int kind, float eps, float *grad_x, ssg_stream_t stream);
int ssg_spsr_branch_loss(const float *branch, const float *gt, int planes, int H, int W, int kind, float eps,
                         void *workspace, double *sum_out, ssg_stream_t stream);
int ssg_spsr_branch_grad(const float *branch, const float *gt, int planes, int H, int W, int kind, float eps,
                         const double *coef, float *grad_branch, ssg_stream_t stream);
int ssg_pixel_sums(const float *pred, const float *target, size_t n, int kind, float eps, void *workspace,
                   double *sum_out, ssg_stream_t stream);
int ssg_pixel_grad(const float *pred, const float *target, size_t n, int kind, float eps, const double *coef,
                   float *grad_pred, ssg_stream_t stream);

/* ---------------------------------------------------------------- (S) ----
 * The EMA and copy updates of a whole parameter set as ONE launch, whatever the number of tensors
 * (basicsr/models/base_model.py:75-82 model_ema and train_BSGRAN/models/model_base.py:192-197 update_E,
 * `ema[k].data.mul_(decay).add_(net[k].data, alpha=1 - decay)` per parameter name; Diffusion-Based-SR's
 * ldm/modules/ema.py LitEma, `shadow.sub_(one_minus_decay * (shadow - param))` per parameter, and its copy_to / store /
 * restore), ssl_amd/csrc/ssg_multi.hip.  Tensors are fp32, walked flat over n elements each; a pair (dst, src) updates
 * dst from src.  Per element, every operation fp32:
 *   SSG_MT_EMA   e <- fmaf(a, p, fl(e d))        d = (float)decay, a = (float)(1 - decay), the subtraction in double:
 *                                                torch's e.mul_(decay).add_(p, alpha=1 - decay), bit for bit
 *   SSG_MT_LIT   e <- e - fl(w fl(e - p))        three roundings, no fma; w = w_dev[0], ONE FLOAT READ ON THE DEVICE
 *                                                (d and a are checked and not used)
 *   SSG_MT_COPY  e <- p                          a move of 32-bit words (d, a and w_dev are checked and not used)
 * Nothing is special-cased: d = 0 with an infinite e gives NaN, as the reference's product does.
 * The table describes the set and lives ON THE DEVICE; the host builds its image once per parameter set and the image
 * is reused from call to call.  8-byte words: {n_tensors, n_chunks, chunk, 0}, then (dst address, src address, n) per
 * tensor, then one word per chunk, tensor index << 32 | index of the chunk inside its tensor, in tensor order and
 * chunk order.  A chunk is ssg_multi_chunk() elements of one tensor (the last chunk of a tensor what is left); an empty
 * tensor has a record and no chunk.
 * ssg_multi_chunks: the set's chunk count, INT_MAX + 1 where it does not fit an int.
 * ssg_multi_table_bytes: the image's size, 32 + 24 n_tensors + 8 chunks; 0 where ssg_multi_table_fill would refuse the
 *   counts.
 * ssg_multi_table_fill: writes the image into `table` (HOST memory, 8-byte aligned) from host arrays of n_tensors dst
 *   addresses, src addresses and element counts.  Touches no device: the addresses are never dereferenced.
 * ssg_multi_apply: ONE launch on `stream` for `table` (the image, on the device) and its n_chunks: a workgroup of 256
 *   threads takes a chunk, and beyond ssg_multi_grid_cap() workgroups takes further chunks grid-stride.  Inside a
 *   chunk accesses are 16 bytes wide behind a scalar head and in front of a scalar tail wherever dst and src share
 *   their alignment mod 16, element by element where they do not: a tensor needs only a float's own alignment.
 *   Stores stay inside [dst, dst + n) of every tensor.  No LDS, no atomics; no allocation, copy, synchronisation or
 *   host read: the call can be captured into a HIP graph.  n_chunks = 0 launches nothing.  The kernel takes the chunk
 *   count from the table: n_chunks only sizes the grid.
 * The caller owns what the table points to: every tensor must be alive and unmoved at each apply, dst ranges must not
 * overlap each other or a src range other than at the same address.
 * Status, decided before the launch with every tensor and the table untouched: SSG_E_BADARG for a null table (or null
 * arrays with n_tensors > 0, or a null address of a non-empty tensor), an unknown kind, a NaN d or a, SSG_MT_LIT without
 * w_dev; SSG_E_ALIGN for a dst or src address of a non-empty tensor that is not 4-byte aligned (detected by the fill), a
 * table that is not 8-byte aligned or a w_dev that is not 4-byte aligned; SSG_E_TOOLARGE for a chunk count (of one
 * tensor or of the set) or a tensor count that does not fit an int; SSG_E_WORKSPACE for a table_bytes below
 * ssg_multi_table_bytes(). */
#define SSG_MT_EMA 0
#define SSG_MT_LIT 1
#define SSG_MT_COPY 2
int ssg_multi_chunk(void);
int ssg_multi_grid_cap(void);
size_t ssg_multi_chunks(size_t n_tensors, const size_t *counts);
size_t ssg_multi_table_bytes(size_t n_tensors, const size_t *counts);
int ssg_multi_table_fill(size_t n_tensors, const size_t *dst, const size_t *src, const size_t *counts,
                         void *table /* host */, size_t table_bytes);
int ssg_multi_apply(const void *table /* device */, size_t n_chunks, int kind, float d, float a,
                    const float *w_dev /* nullable */, ssg_stream_t stream);

/* ---------------------------------------------------------------- (T) ----
 * BSRGAN's degradation chain on a RAGGED batch (GAN-Based-SR/train_BSGRAN/utils/utils_blindsr.py: degradation_bsrgan
 * :443-530, _nocrop :532-616, _ours_p :618-706, _plus :708-792, called once per sample by data/dataset_blindsr.py,
 * dataset_blindsrmask.py and dataset_blindsroursp.py), ssl_amd/csrc/ssg_blindsr.hip.  Every image has its own stage
 * order and its own intermediate sizes, so a launch is driven by one record per image, and there is one launch per
 * operation family and stage slot, whatever the batch.  Images are fp32 planar (C, h, w), C 1 or 3, at ELEMENT offsets
 * of the launch's `in` and `out` buffers (the two ping-pong arenas; both may be one allocation).
 *   SSG_BSR_CONV    add_blur :335-346 and downsample2's shifted kernel :497-501:
 *                   scipy.ndimage.convolve(img, k[:, :, None], mode='mirror')[0::stride, 0::stride], a true convolution
 *                   (the kernel is flipped), out[y, x] = sum_ij k[i, j] in[fold(y stride + r - i), fold(x stride + r - j)],
 *                   r = k / 2, fold the reflection of period 2 (n - 1) that does not repeat the edge sample (n = 1: 0).
 *                   op = k, odd 3 .. 9, its k k fp32 taps row-major at pool_off; stride 1 .. 4; oh = ceil(h / stride).
 *                   One fmaf per tap, row by row of the window: within (k k + 2) 2^-24 sum |k_ij| |x_ij| of fp64.
 *   SSG_BSR_RESIZE  cv2.resize(img, (ow, oh), interpolation=op) of a float32 image, :357, :471, :495, :506, :784.
 *                   Source coordinate (d + 0.5) (n_src / n_dst) - 0.5 in fp64, cast to float, split into floor and
 *                   fraction; fp32 weights; the horizontal taps of a source row are summed first, then the rows.
 *                   SSG_BSR_LINEAR two taps, fraction 0 and index clamped at either end; SSG_BSR_CUBIC four taps, A =
 *                   -0.75, indices clamped; SSG_BSR_AREA: both ratios >= 1 and both integer, the box sum times
 *                   1 / area; both >= 1 otherwise, OpenCV's area table (cell [d s, d s + s), width min(s, n - d s), end
 *                   weights kept above 1e-3, not renormalised); otherwise its area-mode linear rule, sx = floor(d s),
 *                   f = (d + 1) - (sx + 1) / s, 0 where <= 0 and its fractional part otherwise.  Equality with cv2.resize
 *                   itself is SUPPOSED (OpenCV is not available to the tests); the tests hold the kernel to an fp64
 *                   restatement of these rules within a bound that counts every rounding.
 *   SSG_BSR_NOISE   the arithmetic of add_Gaussian_noise :363-377, add_speckle_noise :380-395 and add_Poisson_noise
 *                   :398-409 around their draws, which are passed in as `field` (C planes at field_off; one plane for
 *                   the gray forms), p0 a scale (1 for a field that is already the noise) or Poisson's `vals`:
 *                     GAUSS_COLOR | _GRAY | _CORR      y = x + fl(n p0), n = f_c | f_0 | sum_j M[c][j] f_j, M the 3 x 3 fp32
 *                                                      matrix at pool_off (numpy's multivariate_normal factor,
 *                                                      transposed) applied to a standard-normal colour field
 *                     SPECKLE_COLOR | _GRAY | _CORR    y = x + fl(x fl(n p0)), x clipped first under SSG_BSR_LEAD_CLIP
 *                     POISSON_RATES                    out_c = fl(q_c p0), q = clip(rint(fl(x 255)), 0, 255) / 255 (float32,
 *                                                      half to even: numpy's bits)
 *                     POISSON_COLOR                    y_c = fl(f_c / p0), f the draw
 *                     POISSON_RATES_GRAY               out_0 = (float)(g p0), g the same quantisation in fp64 of
 *                                                      fma(q_2, 0.114, fma(q_1, 0.587, 0.299 q_0)), the fused chain of
 *                                                      numpy's dot: ONE plane is written
 *                     POISSON_GRAY                     y_c = (float)(q_c + (fl(f_0 / p0) - g)), fp64 as numpy promotes it
 *                   oh = h, ow = w; the _CORR and gray Poisson forms need C = 3.  Bit-equal to numpy on the same fields.
 * SSG_BSR_CLIP in flags: np.clip(y, 0, 1) closes the operation (a NaN passes through, as in numpy).
 * The table lives ON THE DEVICE; ssg_blindsr_table_fill writes its image into HOST memory (4-byte aligned,
 * ssg_blindsr_table_bytes(n_images) = 16 + 4 roundup4(n_images + 1) + 64 n_images) from n_images records, and CHECKS them:
 * every range inside in_elems / out_elems / field_elems / pool_elems (the buffers' sizes in elements), no two outputs
 * overlapping, and with same_buffer != 0 no output overlapping any input.  It computes tile0 and tiles_x and returns the
 * launch's tile count.  Words: {n_images, n_tiles, family, 0}, the first tile of every image (n_images + 1 words, padded
 * to four), the records.  A workgroup of 256 threads takes a tile (8 x 32 output pixels of every channel; for noise
 * 1,024 pixels), the image by binary search in the prefix, and beyond ssg_blindsr_grid_cap() workgroups further tiles
 * grid-stride.  Every output element has exactly one writer and there are no atomics: the bits of image b do not depend
 * on the rest of the batch.  The launches allocate, copy and synchronise nothing.
 * ssg_blindsr_tile: the tile of a family, (8, 32) output pixels for conv and resize, (1, 1024) pixels for noise.
 * Status: SSG_E_BADARG for a null pointer, an unknown family / op / flag, C not 1 or 3, an empty image, a kernel size or
 * stride outside the range, sizes that contradict the operation, a NaN p0, overlapping ranges; SSG_E_WORKSPACE for a
 * range that leaves its buffer or a table_bytes below ssg_blindsr_table_bytes(); SSG_E_TOOLARGE for an image or a tile
 * count beyond INT_MAX or a buffer beyond 2^32 - 1 elements; SSG_E_ALIGN for a misaligned pointer. */
#define SSG_BSR_CONV 0
#define SSG_BSR_RESIZE 1
#define SSG_BSR_NOISE 2
#define SSG_BSR_LINEAR 1          /* cv2's interpolation numbers */
#define SSG_BSR_CUBIC 2
#define SSG_BSR_AREA 3
#define SSG_BSR_CLIP 1
#define SSG_BSR_LEAD_CLIP 2
#define SSG_BSR_GAUSS_COLOR 0
#define SSG_BSR_GAUSS_GRAY 1
#define SSG_BSR_GAUSS_CORR 2
#define SSG_BSR_SPECKLE_COLOR 3
#define SSG_BSR_SPECKLE_GRAY 4
#define SSG_BSR_SPECKLE_CORR 5
#define SSG_BSR_POISSON_RATES 6
#define SSG_BSR_POISSON_COLOR 7
#define SSG_BSR_POISSON_RATES_GRAY 8
#define SSG_BSR_POISSON_GRAY 9
typedef struct ssg_blindsr_record {
  unsigned in_off, out_off;   /* elements into `in` / `out` */
  int C, h, w, oh, ow;
  int op;                     /* conv: k; resize: SSG_BSR_LINEAR | CUBIC | AREA; noise: SSG_BSR_GAUSS_COLOR ... */
  int stride;                 /* conv only */
  int flags;                  /* SSG_BSR_CLIP | SSG_BSR_LEAD_CLIP */
  unsigned pool_off;          /* floats into `pool`: the taps or the 3 x 3 matrix */
  unsigned field_off;         /* elements into `field` (noise) */
  float p0;                   /* noise: scale or vals */
  int tile0, tiles_x;         /* written by ssg_blindsr_table_fill */
  int reserved;
} ssg_blindsr_record;
int ssg_blindsr_grid_cap(void);
int ssg_blindsr_tile(int family, int *tile_rows, int *tile_cols);
size_t ssg_blindsr_table_bytes(int n_images);
int ssg_blindsr_table_fill(int family, const ssg_blindsr_record *records, int n_images, size_t in_elems,
                           size_t out_elems, size_t field_elems, size_t pool_elems, int same_buffer,
                           void *table /* host */, size_t table_bytes, int *n_tiles_out);
int ssg_blindsr_conv(const void *table /* device */, int n_tiles, const float *in, float *out, const float *pool,
                     ssg_stream_t stream);
int ssg_blindsr_resize(const void *table /* device */, int n_tiles, const float *in, float *out, ssg_stream_t stream);
int ssg_blindsr_noise(const void *table /* device */, int n_tiles, const float *in, float *out,
                      const float *field /* nullable */, const float *pool /* nullable */, ssg_stream_t stream);

/* ---------------------------------------------------------------- (U) ----
 * A pixel criterion over a RAGGED SET of tensor pairs, one launch each way: the VGG perceptual loss outside its network
 * (GAN-Based-SR/basicsr/losses/basic_loss.py:212-251, `percep_loss += criterion(x_features[k], gt_features[k]) *
 * layer_weights[k]` per tapped layer, and the same over the Gram matrices; train_BSGRAN/models/loss.py:114-130),
 * ssl_amd/csrc/ssg_mcrit.hip.  Pair k is (x_k, g_k) of n_k >= 1 fp32 elements with the weight w_k; d = x_k[i] - g_k[i].
 *   kinds  SSG_PIX_L1, SSG_PIX_MSE, SSG_PIX_CHARBONNIER: l and l' of section (R), the same device functions.
 *          SSG_PIX_FRO (these entry points only): l = d d, the pair's term sqrt(S_k), l' = d.
 *   ssg_mcrit_sums   S_k = sum_i l(d_i) to sums_out[k], k < n_tensors, and sum_k w_k S_k (FRO: sum_k w_k sqrt(S_k)) to
 *          sums_out[n_tensors]: n_tensors + 1 DOUBLES ON THE DEVICE.  The caller puts 1 / n_k into w_k for a mean.  One
 *          launch over the chunks of all pairs (a chunk is ssg_mcrit_chunk() elements of ONE tensor; a workgroup of 256
 *          threads takes a chunk, and beyond ssg_mcrit_grid_cap() workgroups further chunks grid-stride), one fp64
 *          partial per chunk in `workspace`, then one launch of one workgroup that folds every tensor's partials in
 *          chunk order and adds the total in pair order.  Every fp32 l is widened and added in fp64 in a fixed order; no
 *          atomics.  S_k is the same bits whichever other pairs are in the call, and from call to call.
 *   ssg_mcrit_grad   grad_k[i] = (float)(c_k (double)l'(d_i)), c_k = coef[0] w_k in fp64; FRO: c_k = coef[0] w_k /
 *          sqrt(S_k), and 0 where S_k = 0 (torch's norm backward).  coef (ONE DOUBLE) and sums (what ssg_mcrit_sums
 *          wrote; read for FRO only) are device memory: no host read.  A pair whose grad address is 0 is skipped and
 *          nothing of it is read or written.  One launch.  With coef[0] w_k formed in fp64, grad_k is ssg_pixel_grad's
 *          bits on the same pair.
 * x, g, grad, counts and weights are HOST arrays of n_tensors entries (addresses as size_t).  The records travel in the
 * kernels' arguments, 16 pairs to a launch; a larger set takes one more launch (of each kind) per 16 pairs.  Inside a
 * chunk accesses are 16 bytes wide behind a scalar head and in front of a scalar tail wherever g_k or grad_k shares
 * x_k's alignment mod 16, element by element where it does not: a tensor needs only a float's own alignment.  Stores
 * stay inside [grad_k, grad_k + n_k).  No allocation, copy, synchronisation or host read.
 * ssg_mcrit_workspace_bytes: 8 bytes per chunk of the set; 0 where the counts would be refused.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer or array (grad
 * addresses excepted), n_tensors < 1, n_k = 0, an unknown kind, an eps that is negative or not finite, a NaN weight;
 * SSG_E_TOOLARGE for a chunk count (of one tensor or of the set) beyond INT_MAX; SSG_E_WORKSPACE for workspace_bytes <
 * ssg_mcrit_workspace_bytes(); SSG_E_ALIGN for an x, g or grad address that is not 4-byte aligned or a workspace,
 * sums_out, sums or coef that is not 8-byte aligned. */
#define SSG_PIX_FRO 3
int ssg_mcrit_chunk(void);
int ssg_mcrit_grid_cap(void);
size_t ssg_mcrit_workspace_bytes(size_t n_tensors, const size_t *counts);
int ssg_mcrit_sums(size_t n_tensors, const size_t *x, const size_t *g, const size_t *counts, const double *weights,
                   int kind, float eps, void *workspace, size_t workspace_bytes, double *sums_out /* device */,
                   ssg_stream_t stream);
int ssg_mcrit_grad(size_t n_tensors, const size_t *x, const size_t *g, const size_t *grad /* entries nullable */,
                   const size_t *counts, const double *weights, int kind, float eps, const double *sums /* device */,
                   const double *coef /* device */, ssg_stream_t stream);

/* ---------------------------------------------------------------- (V) ----
 * The criteria of the LPIPS (v0.1) and DISTS validation metrics outside their networks, over a RAGGED SET of feature
 * pairs in one launch each plus one finishing launch, ssl_amd/csrc/ssg_featmetric.hip.  Layer k holds n_images fp32
 * NCHW contiguous maps of (C[k], H[k], W[k]) on either side; a map needs only a float's alignment.  Every sum is fp64, of
 * products of two fp32 factors formed in fp64, in a fixed order: no atomics, no scratch, one partial per work unit in
 * `workspace`, folded in unit order.  Results are the same bits from call to call; image n of a batch gives the bits of
 * the image alone; a layer's partials are the same bits whichever other layers are in the call.
 *   ssg_lpips_layers   per pixel d = sum_c w_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2, n = sqrt(sum_c f_c^2), formed
 *          in ONE pass over the channels as A i0^2 - 2 B i0 i1 + Cc i1^2 (A = sum w f0^2, B = sum w f0 f1, Cc = sum w f1^2,
 *          i = 1 / (n + 1e-10)) in fp64, 0 where that is negative.  Identical inputs give exactly 0, an all-zero vector
 *          contributes 0 as the package's 0 / (0 + eps) does, a NaN reaches its own image's results.  w[k] is the layer's
 *          1x1 convolution, C[k] floats on the device.  out (device, n_images x (n_layers + 1) doubles): out[n][k] the
 *          spatial mean of d, out[n][n_layers] their sum in layer order.  A work unit is up to ssg_featmetric_unit()
 *          pixels of one image of one layer (fewer for a layer of fewer pixels: the power of two at or above H W, its
 *          channels split over the rest of the workgroup); at most ssg_featmetric_grid_cap() workgroups, grid-stride
 *          beyond.  Workspace: 8 bytes per unit.
 *   ssg_lpips_layers_backward   the gradient of sum_n coef[n] out[n][n_layers] with respect to both sets of maps, in ONE
 *          launch for all layers and both sides and without a workspace: the adjoint of the UNCLAMPED d (the forward's
 *          clamp of rounding-negative values has no counterpart).  With the forward's five fp64 sums per pixel, n_s =
 *          sqrt(P_s), i_s = 1 / (n_s + 1e-10) and s = coef[n] / (H W):
 *            g0_c = s 2 i0 (w_c (f0_c i0 - f1_c i1) - (A i0 - B i1) (i0 / n0) f0_c)
 *            g1_c = s 2 i1 (w_c (f1_c i1 - f0_c i0) - (Cc i1 - B i0) (i1 / n1) f1_c)
 *          every product and sum in fp64 from the exact fp32 inputs, one cast to fp32 at the store.  The forward's work
 *          units; each walks its channels twice (the sums, then the stores).  coef: n_images floats on the device.
 *          grad0, grad1: HOST arrays of n_layers device addresses of fp32 maps shaped as f0 / f1 (they may not overlap
 *          the inputs); either WHOLE array may be NULL where that side wants no gradient.  One writer per element, no
 *          atomics: the same bits from call to call, image n alone or in a batch, whichever other layers are in the
 *          call.  Identical inputs give exactly +-0 everywhere.  REPRODUCED ON PURPOSE: a pixel whose own vector is all
 *          zero (n_s = 0) gets NaN on that side's C elements of that pixel (0 * inf, what torch's autograd gives through
 *          sqrt's backward at 0) while the other side stays finite there.  A NaN input stays inside its own image.
 *          Status: SSG_E_BADARG also for a NULL coef, both grad arrays NULL, or a null address inside a given grad
 *          array; SSG_E_ALIGN for coef or a gradient address that is not 4-byte aligned; the rest as ssg_lpips_layers.
 *   ssg_dists_score    per (image, layer, channel) plane the sums of x, y, x^2, y^2, x y over chunks of
 *          ssg_featmetric_chunk() elements of ONE plane (5 doubles per chunk in `workspace`, chunks ordered layer, image,
 *          channel, chunk of the plane), then mx = Sx / HW, vx = Sxx / HW - mx^2, cov = Sxy / HW - mx my, S1 = (2 mx my +
 *          c1) / (mx^2 + my^2 + c1), S2 = (2 cov + c2) / (vx + vy + c2), c1 = c2 = 1e-6; alpha, beta: sum_k C[k] floats on
 *          the device, layer after layer.  out (device, n_images x 3 doubles): {1 - (s1 + s2) / ws, s1 / ws, s2 / ws}
 *          with s1 = sum alpha_c S1, s2 = sum beta_c S2, ws = sum alpha + sum beta, channels in a fixed order.
 * f0, f1, w, x, y are HOST arrays of n_layers device addresses (as size_t); C, H, W HOST arrays of n_layers ints.  The
 * records travel in the kernels' arguments.  No allocation, copy, synchronisation or host read.
 * ssg_*_workspace_bytes: 0 where the shapes would be refused.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer, array or address,
 * n_layers outside 1 .. 16, n_images < 1, C, H or W < 1; SSG_E_TOOLARGE for H W or a unit / chunk count beyond INT_MAX;
 * SSG_E_WORKSPACE for workspace_bytes below the reported size; SSG_E_ALIGN for a float address that is not 4-byte
 * aligned or a workspace or out that is not 8-byte aligned. */
int ssg_featmetric_grid_cap(void);
int ssg_featmetric_unit(void);
int ssg_featmetric_chunk(void);
size_t ssg_lpips_workspace_bytes(int n_layers, int n_images, const int *C, const int *H, const int *W);
int ssg_lpips_layers(int n_layers, int n_images, const size_t *f0, const size_t *f1, const size_t *w, const int *C,
                     const int *H, const int *W, void *workspace, size_t workspace_bytes, double *out /* device */,
                     ssg_stream_t stream);
int ssg_lpips_layers_backward(int n_layers, int n_images, const size_t *f0, const size_t *f1, const size_t *w, const int *C,
                              const int *H, const int *W, const float *coef /* device */,
                              const size_t *grad0 /* nullable */, const size_t *grad1 /* nullable */,
                              ssg_stream_t stream);
size_t ssg_dists_workspace_bytes(int n_layers, int n_images, const int *C, const int *H, const int *W);
int ssg_dists_score(int n_layers, int n_images, const size_t *x, const size_t *y, const int *C, const int *H,
                    const int *W, const float *alpha /* device */, const float *beta /* device */, void *workspace,
                    size_t workspace_bytes, double *out /* device */, ssg_stream_t stream);

/* ---------------------------------------------------------------- (W) ----
 * What surrounds the Diffusion fork's U-Net (Diffusion-Based-SR/ldm/models/diffusion/ddpm.py and ddpmssl.py), outside
 * the network, ssl_amd/csrc/ssg_diffusion.hip: the per-sample linear combinations of the schedule, p_sample behind the
 * network call, the training criterion of p_losses, and the tile gather / weighted stitch of p_mean_variance_canvas.
 * Tensors are (B, n) fp32 contiguous, B >= 1, n >= 1; a sample's base needs only a float's alignment.  t is B int64 ON
 * THE DEVICE, every table T fp32 on the device; tab[t_b] is gathered by the kernels and NO entry point reads t on the
 * host.  A t_b outside [0, T) reads nothing: that sample's coefficients, and so its results, are NaN.  Every fp32
 * operation is rounded on its own, in the reference's order (no fma): on the same tables the elementwise results are
 * torch's bits.  A chunk is ssg_diff_chunk() elements of ONE sample; at most ssg_diff_grid_cap() workgroups of 256
 * threads, further chunks grid-stride.  One writer per output element, no atomics, no scratch, no allocation, copy,
 * synchronisation or host read; results are the same bits from call to call, and sample b of a batch gives the bits
 * of that sample alone (for ssg_diff_loss_finish: its S_b).
 *   ssg_diff_combine   out = fl(fl(A[t_b] x) + fl(Bt[t_b] y)) (subtract != 0: -), then, clamp != 0, the clamp to [lo, hi]
 *          (a NaN stays).  q_sample, get_v, predict_start_from_noise, predict_start_from_z_and_v, q_posterior's mean.
 *   ssg_diff_p_sample  x_recon = fl(fl(ra[t_b] x) - fl(rb[t_b] model_out)) for SSG_DIFF_EPS (ra, rb = sqrt_recip_ /
 *          sqrt_recipm1_alphas_cumprod) and SSG_DIFF_V (sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod), model_out
 *          for SSG_DIFF_X0 (ra, rb unused, may be NULL); clip != 0: clamped to [-1, 1]; mean = fl(fl(c1[t_b] x_recon) +
 *          fl(c2[t_b] x)); out = fl(mean + fl(fl(m_b sigma[t_b]) noise)), m_b = (t_b != 0); x_recon to x0_out (nullable).
 *   ssg_diff_loss_sums   one fp64 partial per chunk of sum_i l(target - pred) in `workspace` (8 bytes per chunk,
 *          ssg_diff_workspace_bytes(B, n)); kind SSG_PIX_L1 (|d|) or SSG_PIX_MSE (d d): l in fp32, widened, added in fp64
 *          in an order that depends on n alone, not on the sample's alignment.
 *   ssg_diff_loss_finish   ONE workgroup, fp64: S_b = the sample's partials in chunk order (sums_out, B doubles); mean_b
 *          = S_b / n; wbar = mean_b(p2[t_b]) (p2 NULL: 1), the weight of EVERY sample -- the reference multiplies its (B,)
 *          loss_simple by a (B, 1, 1, 1) weight, and the mean of the (B, 1, 1, B) result is this (ddpmssl.py:397-401);
 *          (with p2 one t_b outside the table therefore makes every sample's results NaN);
 *          l_b = wbar mean_b / exp(logvar[t_b]) + logvar[t_b];
 *          scalars_out (4 doubles) = {loss_simple = mean_b(mean_b), loss_gamma = mean_b(l_b), loss_vlb =
 *          mean_b(lvlb[t_b] mean_b), loss = l_simple_weight loss_gamma + original_elbo_weight loss_vlb}, the reference's
 *          loss_dict; coef_out[b] = dloss / dmean_b = (l_simple_weight wbar / exp(logvar[t_b]) + original_elbo_weight
 *          lvlb[t_b]) / B; dlogvar_out (nullable, T doubles) = dloss / dlogvar, the samples of equal t added IN SAMPLE
 *          ORDER, 0 for a tau no sample has.  All outputs device memory.
 *   ssg_diff_loss_grad   grad_pred[b, i] = (float)(g[0] coef[b] / n (double)(-l'(d))) - fl(rb[t_b] grad_x0[b, i]);
 *          g (ONE FLOAT, the upstream gradient of the loss) and coef are read on the device.  grad_x0 (nullable): the
 *          gradient that arrives through x0 = predict_start_from_noise(x_noisy, t, pred), rb = sqrt_recipm1_alphas_
 *          cumprod; without it rb, t and T are unused.  l' of section (R): L1's is 0 at +-0.
 *   ssg_diff_canvas_gather   out[(k B + b), c, y, x] = src[b, c, oy_k + y, ox_k + x]: ntiles B tiles of (C, ts, ts).
 *   ssg_diff_canvas_stitch   out (B, C, h, w): per element, over the tiles that cover it IN TABLE ORDER, acc =
 *          (float)((double)acc + (double)p w), cnt = (float)((double)cnt + w), out = acc / cnt in fp32 (NaN where no tile
 *          covers): torch's in-place add of an fp64 product into an fp32 tensor.  p is element (c, y - oy_k, x - ox_k) of
 *          tile preds[src_k + b bstep] (bstep 0: one tile for every sample, 1: a tile per sample), preds holding n_preds
 *          tiles; w is weights[b wsb + c wsc + (y - oy_k) ts + (x - ox_k)], fp64 on the device, the caller's strides in
 *          elements (0, 0: one plane), or 1 with weights NULL (an unweighted average).
 * tiles: ntiles records {oy, ox, src} of three ints ON THE DEVICE.  A record whose square leaves the canvas or whose
 * src + b bstep leaves [0, n_preds) is skipped by the kernels: nothing outside the tensors is read or written.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer (those marked nullable
 * excepted), B, n, T, C, h, w, ts or ntiles < 1, ts > h or w, an unknown kind or param, a lo, hi, l_simple_weight or
 * original_elbo_weight that is a NaN, lo > hi, bstep outside {0, 1}; SSG_E_TOOLARGE for a chunk count beyond INT_MAX, B
 * beyond INT_MAX (ssg_diff_loss_finish) or a canvas or tile tensor of 2^31 elements or more; SSG_E_WORKSPACE for
 * workspace_bytes < ssg_diff_workspace_bytes(B, n) (which is 0 where B and n would be refused); SSG_E_ALIGN for a float
 * address that is not 4-byte aligned or a t, workspace, weights or double address that is not 8-byte aligned. */
#define SSG_DIFF_EPS 0
#define SSG_DIFF_X0 1
#define SSG_DIFF_V 2
int ssg_diff_chunk(void);
int ssg_diff_grid_cap(void);
size_t ssg_diff_workspace_bytes(size_t B, size_t n);
int ssg_diff_combine(const float *x, const float *y, const long long *t, const float *A, const float *Bt, int T,
                     size_t B, size_t n, int subtract, int clamp, float lo, float hi, float *out, ssg_stream_t stream);
int ssg_diff_p_sample(const float *x, const float *model_out, const float *noise, const long long *t, const float *ra,
                      const float *rb, const float *c1, const float *c2, const float *sigma, int T, size_t B, size_t n,
                      int param, int clip, float *out, float *x0_out /* nullable */, ssg_stream_t stream);
int ssg_diff_loss_sums(const float *pred, const float *target, size_t B, size_t n, int kind, void *workspace,
                       size_t workspace_bytes, ssg_stream_t stream);
int ssg_diff_loss_finish(const void *workspace, size_t workspace_bytes, const long long *t,
                         const float *p2 /* nullable */, const float *logvar, const float *lvlb, int T, size_t B,
                         size_t n, double l_simple_weight, double original_elbo_weight, double *sums_out,
                         double *scalars_out, double *coef_out, double *dlogvar_out /* nullable */,
                         ssg_stream_t stream);
int ssg_diff_loss_grad(const float *pred, const float *target, const float *grad_x0 /* nullable */,
                       const long long *t, const float *rb, int T, const float *g /* device */,
                       const double *coef /* device */, size_t B, size_t n, int kind, float *grad_pred,
                       ssg_stream_t stream);
int ssg_diff_canvas_gather(const float *src, const int *tiles /* device */, int ntiles, int B, int C, int h, int w,
                           int ts, float *out, ssg_stream_t stream);
int ssg_diff_canvas_stitch(const float *preds, int n_preds, int bstep, const int *tiles /* device */, int ntiles,
                           const double *weights /* nullable */, size_t wsb, size_t wsc, int B, int C, int h, int w,
                           int ts, float *out, ssg_stream_t stream);

/* ---------------------------------------------------------------- (X) ----
 * The Adam / AdamW step of a whole parameter group as ONE launch, whatever the number of tensors (torch.optim.Adam and
 * AdamW as basicsr/models/base_model.py:103-120 get_optimizer, train_BSGRAN/models/model_ssl.py:229-230 and the
 * Diffusion fork's configure_optimizers build them), ssl_amd/csrc/ssg_multi.hip.  Tensors are fp32, walked flat over n
 * elements each; tensor i is (p, g, m, v): parameter, gradient, exp_avg, exp_avg_sq.  Per element, every operation
 * fp32 and rounded on its own (no fma), `/` and sqrtf correctly rounded:
 *   g' = g                               SSG_ADAM_PLAIN
 *   g' = fl(g + fl(wd p))                SSG_ADAM_L2         Adam's weight decay
 *   p' = fl(p cwd)                       SSG_ADAM_DECOUPLED  AdamW's; p' = p otherwise
 *   m  <- fl(m + fl(w1 fl(g' - m)))
 *   v  <- fl(fl(v b2) + fl(w2 fl(g' g')))
 *   den = fl(fl(sqrtf(v) / s2) + eps)
 *   p  <- fl(p' - fl(a fl(m / den)))
 * Nothing is special-cased: NaN and infinite gradients propagate as the formulas say.  This is torch's single-tensor
 * Adam operation by operation, NOT torch's bits: torch's lerp_ and vectorised multiply-adds round differently in a
 * share of the elements (tests/adam_reference.py holds both to an fp64 evaluation).
 * The scalars are formed by the caller in double, by torch's expressions, and cast to float once each: a = lr / (1 -
 * beta1^t), w1 = 1 - beta1, b2 = beta2, w2 = 1 - beta2, s2 = (1 - beta2^t)^0.5, cwd = 1 - lr wd.  They travel in the
 * launch's arguments, so a changed lr or t changes no table; and a HIP graph that captured the call would replay step
 * t's scalars: DO NOT capture it (torch's Adam without `capturable` has the same limit).
 * The table is section (S)'s with four words per tensor, {n_tensors, n_chunks, chunk, 0}, then (p address, m address,
 * v address, n) per tensor, then one word per chunk; the g addresses are an array of n_tensors 8-byte words OF THEIR
 * OWN, `grads`: gradients move between steps under zero_grad(set_to_none=True), and a moved gradient costs a new image
 * of that array, not of the table.  Both live ON THE DEVICE at the apply; the fills write host images.
 * The chunk size, the grid cap and the set's chunk count are section (S)'s: ssg_multi_chunk(), ssg_multi_grid_cap(),
 *   ssg_multi_chunks().
 * ssg_adam_table_bytes: the table image's size, 32 + 32 n_tensors + 8 chunks; 0 where ssg_adam_table_fill would refuse
 *   the counts.  The grads image is 8 n_tensors bytes.
 * ssg_adam_table_fill: writes both images (HOST memory, 8-byte aligned) from host arrays of addresses and counts.
 * ssg_adam_grads_fill: writes the grads image alone, for new g addresses and the filled HOST table image of the same
 *   set; the new addresses are checked against the image's p, m and v ranges.  Neither touches a device.
 * ssg_adam_apply: ONE launch on `stream`: a workgroup of 256 threads takes a chunk, beyond ssg_multi_grid_cap()
 *   workgroups further chunks grid-stride.  p is accessed 16 bytes wide behind a scalar head and in front of a scalar
 *   tail; g, m and v 16 bytes wide where all three share p's alignment mod 16 and element by element otherwise (one
 *   decision per chunk).  Stores stay inside [p, p + n), [m, m + n) and [v, v + n) of every tensor; g is only read.
 *   No LDS, no atomics, no scratch; no allocation, copy, synchronisation or host read.  n_chunks = 0 launches nothing.
 * The caller owns what the images point to: every tensor must be alive and unmoved at each apply.
 * Status, decided before the launch with every tensor and both images untouched: SSG_E_BADARG for a null image or
 * scalars (or null arrays with n_tensors > 0, or a null address of a non-empty tensor), two of the 4 n_tensors ranges
 * of the non-empty tensors that overlap, a table image of another tensor count (ssg_adam_grads_fill), an unknown mode;
 * SSG_E_ALIGN for an address of a non-empty tensor or a scalars address that is not 4-byte aligned, an image that is
 * not 8-byte aligned; SSG_E_TOOLARGE for a chunk count (of one tensor or of the set) or a tensor count that does not
 * fit an int; SSG_E_WORKSPACE for a table_bytes below ssg_adam_table_bytes() or a grads_bytes below 8 n_tensors. */
#define SSG_ADAM_PLAIN 0
#define SSG_ADAM_L2 1
#define SSG_ADAM_DECOUPLED 2
typedef struct ssg_adam_scalars {
  float a, w1, b2, w2, s2, eps;
  float wd;  /* SSG_ADAM_L2 only */
  float cwd; /* SSG_ADAM_DECOUPLED only */
  int mode;  /* SSG_ADAM_* */
} ssg_adam_scalars; /* 36 bytes */
size_t ssg_adam_table_bytes(size_t n_tensors, const size_t *counts);
int ssg_adam_table_fill(size_t n_tensors, const size_t *p, const size_t *g, const size_t *m, const size_t *v,
                        const size_t *counts, void *table /* host */, size_t table_bytes, void *grads /* host */,
                        size_t grads_bytes);
int ssg_adam_grads_fill(const void *table /* host */, size_t n_tensors, const size_t *g, void *grads /* host */,
                        size_t grads_bytes);
int ssg_adam_apply(const void *table /* device */, const void *grads /* device */, size_t n_chunks,
                   const ssg_adam_scalars *scalars /* host */, ssg_stream_t stream);

/* ---------------------------------------------------------------- (Y) ----
 * Spectral normalisation of a whole set of layers in a fixed handful of launches, whatever the number of layers
 * (torch.nn.utils.spectral_norm with dim = 0, n_power_iterations = 1, eps = 1e-12, as basicsr's UNetDiscriminatorSN and
 * KAIR's Discriminator_UNet / Discriminator_PatchGAN / Discriminator_VGG_128_SN wrap their layers in it),
 * ssl_amd/csrc/ssg_specnorm.hip.  Additive: ssg_abi_version() stays 6.  Layer l is (W, u, v): W fp32, R x K row-major
 * (a contiguous conv weight: out x in kh kw), u (R) and v (K) fp32.  Training-mode forward:
 *   t = W^T u      v <- (float)(t / max(|t|, eps))     stored in place and into the call's saved block
 *   s = W v        u <- (float)(s / max(|s|, eps))     (from the fp32 v) stored in place and saved
 *   sigma = u . s  (fp32 u, fp64 s)    sigma32 = (float)sigma saved    out = W / sigma32, one fp32 division per element
 * Eval mode skips the two updates and uses u, v as stored (the saved block is filled all the same).  Backward, with G the
 * gradient with respect to out:  dW = (float)((G - <G, W / sigma32> u v^T) / sigma32), in fp64 from the call's SAVED u,
 * v and sigma32; a layer whose G address is 0 is skipped and its part of the gradient block is left as it was.
 * Every product of two fp32 values is exact in fp64 and every sum is fp64 in an order fixed by index: the same bits from
 * call to call, for a layer alone or among others, at any 4-byte alignment.  max(x, eps) keeps a NaN; an all-zero W
 * gives u = v = 0 and out = NaN, as torch does.  A NaN in one layer stays in that layer.
 * The table image (8-byte words, HOST memory from ssg_sn_table_fill, then copied to the device by the caller):
 *   {n_layers, units of launch A, units of launch B, chunks, chunk, floats of the output block, doubles of the
 *   workspace, floats of the saved block}; per layer eight words {W, u, v addresses, R, K, the layer's offset into the
 *   output block (floats, a multiple of 64; the gradient block has the same layout), into the workspace (doubles), into
 *   the saved block (floats: u, then v, then sigma32)}; three prefix tables of n_layers + 1 words (the first unit of
 *   each layer in A, in B, and its first chunk).  The output, workspace and saved blocks are the CALLER's, per call:
 *   ssg_sn_output_bytes, ssg_sn_workspace_bytes, ssg_sn_saved_bytes (0 where the fill would refuse the shapes).  The
 *   workspace is only scratch between the launches of one call.
 * ssg_sn_forward: three launches on `stream` (training) or two (eval) for `table` (the image on the device) and `image`
 *   (the same image on the host, from which sizes and grids are read).  A unit of launch A is ssg_sn_strip() columns by
 *   ssg_sn_rows_a() rows, of launch B ssg_sn_rows_b() rows, of launch C ssg_sn_chunk() elements; grids are capped at
 *   ssg_sn_grid_cap() workgroups of 256 threads and walk grid-stride.  No atomics, no scratch; LDS holds the four wave
 *   sums of a fold.  No allocation, copy, synchronisation or host read of device memory: it may be captured.
 * ssg_sn_backward: two launches; `grads` is a DEVICE array of n_layers 8-byte words, the G addresses (0: no gradient);
 *   `saved` the block of the forward call it belongs to; `grad` a block laid out as the output block.
 * The caller owns what the image points to: every tensor must be alive and unmoved at each call.
 * Status, decided before any launch with every tensor untouched: SSG_E_BADARG for a null pointer or array, R or K < 1,
 * a training flag other than 0 or 1, a null address, or two of the 3 n_layers ranges (W, u, v) that overlap;
 * SSG_E_ALIGN for a tensor address or block that is not 4-byte aligned, a table, image, workspace or grads array that is
 * not 8-byte aligned; SSG_E_TOOLARGE for a layer count, a layer of 2^31 elements and more, or a unit count beyond
 * INT_MAX; SSG_E_WORKSPACE for a table_bytes below ssg_sn_table_bytes() or an output, gradient, workspace or saved
 * block smaller than the image says. */
int ssg_sn_chunk(void);
int ssg_sn_grid_cap(void);
int ssg_sn_strip(void);
int ssg_sn_rows_a(void);
int ssg_sn_rows_b(void);
size_t ssg_sn_table_bytes(size_t n_layers, const size_t *rows, const size_t *cols);
size_t ssg_sn_output_bytes(size_t n_layers, const size_t *rows, const size_t *cols);
size_t ssg_sn_workspace_bytes(size_t n_layers, const size_t *rows, const size_t *cols);
size_t ssg_sn_saved_bytes(size_t n_layers, const size_t *rows, const size_t *cols);
int ssg_sn_table_fill(size_t n_layers, const size_t *w, const size_t *u, const size_t *v, const size_t *rows,
                      const size_t *cols, void *table /* host */, size_t table_bytes);
int ssg_sn_forward(const void *table /* device */, const void *image /* host */, int training, float *out,
                   size_t out_bytes, void *workspace, size_t workspace_bytes, float *saved, size_t saved_bytes,
                   ssg_stream_t stream);
int ssg_sn_backward(const void *table /* device */, const void *image /* host */, const void *grads /* device */,
                    const float *saved, size_t saved_bytes, float *grad, size_t grad_bytes, void *workspace,
                    size_t workspace_bytes, ssg_stream_t stream);

/* ---------------------------------------------------------------- (Z) ----
 * SwinIR's (shifted-)window attention between a block's qkv and proj Linears (GAN-Based-SR/basicsr/archs/swinir_arch.py:
 * WindowAttention inside SwinTransformerBlock), ssl_amd/csrc/ssg_winattn.hip.  Additive: ssg_abi_version() stays 6.
 * Window 8 (64 tokens), C = heads head_dim, 1 <= head_dim <= 32.
 *   qkv   (B, H, W, 3 C) fp32: the qkv Linear applied to the UNPARTITIONED token grid; element
 *         [b, y, x, (s heads + h) head_dim + c] is q, k, v for s = 0, 1, 2 (the memory of the reference's
 *         reshape(b_, n, 3, heads, d)).  dqkv likewise.
 *   bias_table (225, heads) fp32, the module's relative_position_bias_table; dbias_table likewise (nullable: not wanted).
 *   out, dout (B, H, W, C) fp32, the layout proj consumes.
 * Token (iy, ix) of window (wy, wx) has the shifted coordinate ys = 8 wy + iy, xs = 8 wx + ix and is read from and
 * written back to ((ys + shift) mod H, (xs + shift) mod W): both rolls, the partition and the merge are index
 * arithmetic.  Per (image, window, head), every fp32 operation rounded on its own:
 *   S_ij = [fma chain over c of fl(q_ic scale) k_jc] + bias_table[(iy_i - iy_j + 7) 15 + (ix_i - ix_j + 7), h]
 *          + (shift > 0: -100 where label_i != label_j, else 0), label = 3 ly + lx, ly = (ys >= H - 8) + (ys >= H - shift)
 *          and lx likewise from xs: calculate_mask's values, with no mask tensor and no relative_position_index read;
 *   P = softmax over j (row maximum subtracted, expf, a sum in an order fixed by index, a division);
 *   O_ic = fma chain over j of P_ij v_jc.
 * ssg_winattn_forward: one launch.  ssg_winattn_backward: P is recomputed from qkv (nothing is saved by the forward);
 *   dv = P^T dO, dP = dO v^T, dS = P o (dP - rowsum(P o dP)), dq = scale dS k, dk = dS^T fl(q scale), every element of dqkv
 *   written once (no zero-fill needed); dbias_table[idx, h] = the sum of dS_ij over the batch, the windows and the pairs
 *   of idx, in fp64 through one partial per workgroup in `workspace` (ssg_winattn_workspace_bytes; only scratch
 *   within the call; not read when dbias_table is NULL) and a second launch that adds them in a fixed order.
 * A workgroup of 256 threads takes one (image, window, head); grids are capped at ssg_winattn_grid_cap() rounded down
 * to a multiple of heads and walk grid-stride.  No atomics, no scratch, no allocation, copy or synchronisation: both
 * may be captured.  The same bits from call to call, for an image alone or in a batch, at any 4-byte alignment; a NaN
 * in a token stays inside its window in out and dqkv.
 * Status, decided before any launch with the outputs untouched: SSG_E_BADARG for a null pointer (dbias_table excepted;
 * workspace only with dbias_table), B, H, W or heads < 1, H or W no multiple of 8, shift outside 0 .. 7, head_dim
 * outside 1 .. 32; SSG_E_ALIGN for a float pointer that is not 4-byte aligned or a workspace that is not 8-byte
 * aligned; SSG_E_TOOLARGE for H W or a unit count beyond INT_MAX; SSG_E_WORKSPACE for workspace_bytes below
 * ssg_winattn_workspace_bytes(...) (which is 0 for a shape that would be refused). */
int ssg_winattn_grid_cap(void);
size_t ssg_winattn_workspace_bytes(int B, int H, int W, int heads, int head_dim);
int ssg_winattn_forward(const float *qkv, const float *bias_table, float *out, int B, int H, int W, int heads,
                        int head_dim, int shift, float scale, ssg_stream_t stream);
int ssg_winattn_backward(const float *qkv, const float *bias_table, const float *dout, float *dqkv,
                         float *dbias_table /* nullable */, void *workspace, size_t workspace_bytes, int B, int H, int W,
                         int heads, int head_dim, int shift, float scale, ssg_stream_t stream);

#ifdef SSG_PROFILE
/* PROFILING BUILD ONLY (libssg_hip_prof.so, compiled with -DSSG_PROFILE; the product library libssg_hip.so does not
 * export this symbol and has no code path that skips work).  Results are WRONG while a mask is set: skip kernel
 * phases or whole launches so that one kernel of a multi-kernel entry point can be timed with events on its stream.
 * Bits: 25 dense-tile forward, 26 direct forward, 27 dense-tile backward, 28 direct backward (split mode), 29 G rows;
 * lower bits ablate phases inside kernels (ssg_api.hip).  Returns the previous mask; 0 = production behaviour.  The
 * environment variable SSG_DEBUG_SKIP presets the mask, in this build only. */
int ssg_set_profile_mask(int mask);
/* workgroups per CU the HIP runtime reports for a kernel at its launch geometry (0: ssg_fwd_strip<49,13,3,3>) */
int ssg_prof_occupancy(int which);
/* ssg_fwd_strip's per-workgroup clocks of its last launch: host[3 i] = start, [3 i + 1] = end (s_memtime; comparable
 * within one XCD only), [3 i + 2] = XCC id << 32 | HW_ID, for the first n / 3 (<= 1024) workgroups */
int ssg_prof_strip_times(unsigned long long *host, int n);
/* on != 0: every launch of the library is preceded by a kernel that fills the LDS of every CU with `pattern` (a kernel
 * that reads an LDS word it has not written then sees the pattern, not a previous workgroup's data: audit of
 * uninitialised LDS reads, tools/r5_poison_suite.sh).  Results stay correct.  Returns the previous switch. */
int ssg_prof_set_lds_poison(int on, unsigned pattern);
#endif

/* Host helper for profiling builds: name of the HIP kernel a configuration
 * dispatches to ("ssg_fwd<25,9,5>", "ssg_fwd_generic", ...). */
const char *ssg_kernel_name(int ks, int kw, int backward);

#ifdef __cplusplus
}
#endif
#endif /* SSG_HIP_H */
