/* centernet_uda_hip.h -- C ABI of libcenternet_uda_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the CenterNet-UDA hot path.  Plain pointers, sizes
 * and a HIP stream; no torch types.  All tensors are contiguous fp32 NCHW in
 * device memory unless a comment says otherwise; index tensors are int64,
 * masks uint8 (the batch schema of datasets/coco.py:168-174,242-251).  All work
 * is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default
 * stream) and nothing synchronises the host -- the reference likewise enqueues
 * on the current stream (libs/DCNv2/src/cuda/dcn_v2_cuda.cu:107,139).
 *
 * Every function returns 0 on success, CNUDA_ERR_INVALID_ARGUMENT (-1) for a
 * rejected argument, or a positive hipError_t for a failed launch;
 * cnuda_last_error() describes the most recent failure on the calling thread.
 * The reference raises C++ exceptions -> Python RuntimeError for the first
 * kind (dcn_v2_cuda.cu:60-64,80-84) and only printf's the second
 * (dcn_v2_im2col_cuda.cu:346-350); the Python shim in
 * centernet-uda_amd/hip_runtime raises RuntimeError for both.
 *
 * Scratch memory is caller-owned: each family has a *_workspace_bytes() query
 * and takes (workspace, workspace_bytes); nothing is allocated or freed inside
 * a call, so every entry point is legal inside hipGraph capture.
 */
#ifndef CENTERNET_UDA_HIP_H
#define CENTERNET_UDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNUDA_ERR_INVALID_ARGUMENT (-1)
#define CNUDA_ABI_VERSION 2

typedef void* cnuda_stream_t; /* hipStream_t */

int cnuda_abi_version(void);
const char* cnuda_last_error(void);

/* Matrix-pipe mode of the convolution / DCN implicit GEMMs (process-wide; no counterpart in the reference,
 * whose cuDNN / cuBLAS calls pick their own algorithm, backends/dla.py:26,34 and dcn_v2_cuda.cu:95-110):
 *   0  f32 MFMA: exact f32 products and f32 accumulation (default);
 *   1  every f32 operand is cut exactly into three bf16 pieces and the product is formed from the six leading
 *      piece products on the bf16 MFMA with f32 accumulation (error per product below 2^-23, one f32 rounding).
 * Initial value from the environment variable CNUDA_MATRIX_MODE.  Returns 0 or CNUDA_ERR_INVALID_ARGUMENT. */
int cnuda_set_matrix_mode(int mode);
int cnuda_get_matrix_mode(void);

/* Pack cache, no counterpart in the reference (cuDNN / cuBLAS keep their own operand layouts).  The implicit GEMMs
 * read the small weight operand from a zero-padded [Kp][Mp] image that used to be rebuilt by a tiny kernel on every
 * convolution call although it only changes when the weights do.  cnuda_pack_cache_attach hands the library ONE
 * caller-owned device arena (nothing is allocated inside the library; NULL detaches and forgets every slot).
 * cnuda_pack_stamp(token, version), called on the calling thread right before a convolution / DCN entry point,
 * names the weights that call will pack: `token` identifies their owner (0 = anonymous: never cached), `version`
 * changes whenever their values may have changed.  A slot is reused iff the same token packed the same source
 * buffer to the same image before and the version is unchanged; the stamp stays in force until the next
 * cnuda_pack_stamp on that thread (callers reset it to (0, 0) after the call).  cnuda_pack_cache_used: bytes taken;
 * cnuda_pack_cache_fills: how often a cached image was (re)written on a convolution's own call (steady state: 0 per call). */
int cnuda_pack_cache_attach(void* arena, size_t bytes);
int cnuda_pack_stamp(unsigned long long token, unsigned long long version);
size_t cnuda_pack_cache_used(void);
unsigned long long cnuda_pack_cache_fills(void);
/* Eviction: slots of modules that no longer exist are never returned one by one; when an image does not fit any more
 * the cache forgets EVERY slot at the start of the next stamped call (the live modules re-pack once) instead of
 * silently not caching for the rest of the process.  cnuda_pack_cache_resets: how often that happened. */
unsigned long long cnuda_pack_cache_resets(void);
/* After an optimizer step that rewrote [params, params + params_bytes) behind the callers' version counters: every
 * cached image whose source lies in that range and that was current in epoch `old_epoch` (the high 32 bits of the
 * version it was stamped with) is rebuilt by ONE launch on `stream` and re-stamped with `new_epoch` (low 32 bits
 * kept).  `table`: >= 96 bytes per cached image of device scratch that stays valid until the next call (the job
 * list; rewritten only when the set of images changes).  No reference counterpart. */
int cnuda_pack_refresh(const void* params, size_t params_bytes, unsigned long long old_epoch,
                       unsigned long long new_epoch, void* table, size_t table_bytes, cnuda_stream_t stream);
/* The same for `ranges` rewritten buffers at once (host arrays params[i], params_bytes[i]): a step that rewrote a
 * student's arena AND a teacher's flat buffer carries both models' images into `new_epoch` with one launch and one
 * table.  ranges == 1 is cnuda_pack_refresh. */
int cnuda_pack_refresh_ranges(const void* const* params, const size_t* params_bytes, int ranges,
                              unsigned long long old_epoch, unsigned long long new_epoch, void* table,
                              size_t table_bytes, cnuda_stream_t stream);

/* Measurement aid (bench.py roofline leg), not part of the reference's surface:
 * cnuda_prof_enable(n) pre-creates n hipEvent pairs; cnuda_prof_arm(tag) makes
 * the NEXT convolution / DCN main-kernel launch record a start/stop pair on its
 * own launch stream; cnuda_prof_collect synchronises on the recorded events and
 * returns (tag, milliseconds, kernel name) triples -- the name is written by the
 * launcher itself (the kernel template instance it selected for that call), in
 * `names` as cap strings of cnuda_prof_name_len() bytes (nullable).  An entry point
 * made of several timed kernels reports them under one tag, told apart by bits 24..
 * of the tag.  Costs nothing when not armed. */
int cnuda_prof_enable(int max_records);
int cnuda_prof_arm(int tag);
int cnuda_prof_collect(int* tags, float* ms, char* names, int cap);
int cnuda_prof_name_len(void);

/* Test aids (tests/test_zz_kernel_coverage.py, tests/test_gpu_dcn.py), not part of the reference's surface.
 * Launch log: while enabled, every kernel launch of the library is counted per kernel; cnuda_launch_log_collect
 * writes one line "<kernel symbol name, demangled, as a rocprofv3 kernel trace shows it>\t<launches so far>" per
 * distinct kernel, in first-launch order, into names[cap] and returns their count (callers diff two snapshots to
 * learn what ran in between).  enable(1) from the disabled state clears the counts.
 * cnuda_dcn_set_fused_min_tiles: cnuda_dcn_v2_backward runs its two data-gradient walks as ONE launch
 * (dcn_bwd_data_kernel + geometry records from dcn_prep_kernel) when the call has at least this many
 * (image, 256-pixel tile) pairs -- 512 by default: the 128 x 128 / 64 x 64 maps of the benched step -- and as two
 * kernels below it.  Tests set 1 to run small geometries (borders, odd widths, out-of-bounds samples) through the
 * one-launch form, and INT_MAX to force the two-kernel form; values < 1 restore the default.  Returns the previous
 * threshold.  Process-wide; results do not depend on it beyond the summation order inside grad_input.
 * cnuda_conv_set_halo_policy: which 3x3 / stride-1 / padding-1 convolutions take the halo-tile kernels (csrc/hconv.cuh):
 * level 0 none, 1 every eligible layer, 2 the 32-row GEMMs (default; initial value from CNUDA_HCONV), and only calls
 * with at least min_tiles 128-pixel tiles (default 128).  Negative level / min_tiles < 1 leave that setting unchanged.
 * Returns level | min_tiles << 8 after the change.  Tests use (1, 1) to run small shapes through every tile variant. */
int cnuda_launch_log_enable(int on);
int cnuda_launch_log_collect(char* names, size_t cap);
int cnuda_dcn_set_fused_min_tiles(int min_tiles);
/* cells of the data-gradient walk's LDS window beyond the undeformed 3x3 footprint (default 2; < 1 restores it).  Returns the
 * previous value.  Samples further out than this are strays (global atomics): a wider window for models whose offsets are
 * pixels, at fewer workgroups per CU.  Measurements and tests; results do not depend on it beyond summation order. */
int cnuda_dcn_set_scatter_margin(int margin);
/* columns of the data-gradient walk's pixel tile (16, 32 or 64; 256 pixels per tile; 0 = by the map width, the default).
 * Returns the previous value.  Measurements only; results do not depend on it beyond summation order. */
int cnuda_dcn_set_walk_tile(int tile_cols);
/* Offset regime of the next cnuda_dcn_v2_* calls (process-wide, the host layer sets it per call): bit 0 -> the data-gradient
 * walk's window takes a margin of 4 cells (many samples beyond +-2 px), bit 1 -> the forward takes the gathering loader
 * instead of the LDS-window kernel (many samples beyond +-3 px).  Returns the previous value.  Speed only: results do not
 * depend on it beyond summation order.  cnuda_dcn_offset_census adds to counts[0] / counts[1] (caller-zeroed) the number
 * of (pixel, tap) samples of `offset` [B][2*taps][HW] that leave +-2 px / +-3 px in either direction. */
int cnuda_dcn_set_offset_regime(int regime);
int cnuda_dcn_offset_census(const float* offset, int B, int taps, long long HW, unsigned* counts, cnuda_stream_t stream);
int cnuda_conv_set_halo_policy(int level, int min_tiles);
/* Split-K of the forward-type convolution GEMMs (forward, stride-1 and parity-class input gradient; csrc/igemm.cuh
 * igemm_fwd_*splitk_kernel): a call whose pixel x row tiles at the natural row tile number fewer than max_tiles (default
 * 128: half the chip) and whose K has at least 32 chunks cuts K over grid.y -- partial slabs in the workspace, a fixed-order
 * reduce with the usual epilogue -- instead of shrinking the row tile.  max_tiles 0 = never; < 0 restores the default.
 * Returns the previous value.  Speed only: results differ by summation order (blocked over the splits).  CNUDA_SPLITK=0
 * disables it for the process. */
int cnuda_conv_set_splitk_policy(int max_tiles);

/* ------------------------------------------------------------------------
 * Detection decode -- replaces backends/decode.py:35-76 (decode_detection),
 * :6-13 (_nms), :16-32 (_topk) and the gathers of utils/tensor.py:10-25.
 *
 *   heat [B,C,H,W]  scores (the callers pass clamp(sigmoid) probabilities,
 *                   uda/base.py:76-77, export.py:31-38)
 *   wh   [B,wh_ch,H,W]  wh_ch = 2, or 3 when rotated (3rd = angle logit)
 *   reg  [B,2,H,W] or NULL (NULL -> +0.5 cell centre, decode.py:49-51)
 *   dets [B,K,6]  = x1,y1,x2,y2,score,class         (rotated == 0)
 *        [B,K,7]  = cx,cy,w,h,angle_deg,score,class  (rotated != 0)
 *   inds [B,K] int64 spatial index y*W+x of every detection, or NULL
 * Order among equal scores (unspecified in torch.topk): score descending, then
 * class ascending, then spatial index ascending.  1 <= K <= min(H*W, 1024).
 * nms_size must be odd (reference default 3).
 * ---------------------------------------------------------------------- */
/* Stage 1 cuts a plane into up to `max_bands` (1, 2 or 4; default 2; < 1 restores it) bands of rows, one workgroup each, when
 * the planes alone would leave CUs idle (B * C * bands <= 512).  Returns the previous value.  Speed only: the result is the
 * same bit for bit (tests/test_gpu_decode.py runs every case with 1, 2 and 4). */
int cnuda_decode_set_max_bands(int max_bands);
/* threads of stage 2's workgroup: 256, 512 or 1024; 0 = the default (1,024).  Returns the previous value.  Measurements; the result does not depend on it. */
int cnuda_decode_set_stage2_threads(int threads);
size_t cnuda_decode_workspace_bytes(int B, int C, int H, int W, int K);
int cnuda_decode_detection(const float* heat, const float* wh, const float* reg,
                           float* dets, int64_t* inds,
                           int B, int C, int H, int W, int K, int wh_ch, int rotated, int nms_size,
                           void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* keypoint branch (decode.py:69-74): out [B,K,J,2] = kps[b, 2j + {0,1}, inds[b,k]] + (xs, ys) with
 * xs = inds % W + reg_x, ys = inds / W + reg_y (reg NULL: + 0.5), the centres of decode.py:44-51 */
int cnuda_decode_keypoints(const float* kps, const float* reg, const int64_t* inds, float* out,
                           int B, int J, int K, int H, int W, cnuda_stream_t stream);
/* _nms alone: out = heat * (1 - ceil(maxpool_k(heat) - heat))  (decode.py:6-13) */
int cnuda_nms(const float* heat, float* out, int B, int C, int H, int W, int nms_size,
              cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * Modulated deformable convolution (DCNv2) -- replaces the native module
 * `_ext` of libs/DCNv2 (src/vision.cpp:4-8):
 *   dcn_v2_forward  (src/dcn_v2.h:10-46  -> cuda/dcn_v2_cuda.cu:42-172)
 *   dcn_v2_backward (src/dcn_v2.h:48-92  -> cuda/dcn_v2_cuda.cu:206-341)
 * Argument order follows the native entry points (input, weight, bias, offset,
 * mask, ...).  offset [B, 2*kh*kw*dg, Ho, Wo] with channel 2*tap = dy and
 * 2*tap+1 = dx (cuda/dcn_v2_im2col_cuda.cu:170-174); mask [B, kh*kw*dg, Ho, Wo].
 * A sample is taken iff -1 < y < H and -1 < x < W, corners outside the plane
 * read 0 (:37-48,180).
 * Scratch: everything lives in the caller's workspace (nothing is allocated inside
 * a call).  forward samples inside the implicit GEMM's loader and materialises no
 * `columns` buffer when the output channels fit one tile of the GEMM; layers whose
 * output channels span several tiles (small feature maps) sample the columns once
 * into the workspace and run a plain GEMM over them.  backward materialises the
 * column gradient dcol[B, kh*kw*C, Ho*Wo] in the workspace (one 1x1 implicit GEMM,
 * two streaming consumers) and a 16-byte geometry record per (pixel, tap).
 * backward writes (does not accumulate into) all five gradients.  grad_input is
 * accumulated in LDS windows with plain read-add-write; fp32 global atomics remain
 * only for the window flush (one per touched cell), for samples that leave their
 * tile's window and for in-instruction collisions -- far fewer than the reference's
 * one atomic per corner (:238-252), but grad_input is still bit-reproducible only up
 * to the order of those.  deformable_group > 1 (round 6): composed of deformable_group = 1 calls on contiguous copies
 * of each group's input channels and weights (offsets / mask and their gradients in place, through their batch strides),
 * the group outputs added in group order -- 64 -> 64 at 128 x 128, B = 32, dg = 2 with the groups' columns saved: 1.18 / 2.90 ms
 * forward / backward against 0.89 / 2.36 ms with one group (rounds 1-5: one thread per element and global atomics, 45 ms /
 * 1.5 s; profiles/r6_dcn_dg2.txt).  Width 1 keeps that plain path.
 * ---------------------------------------------------------------------- */
size_t cnuda_dcn_v2_workspace_bytes(int B, int C, int H, int W, int Cout, int kh, int kw,
                                    int sh, int sw, int ph, int pw, int dh, int dw, int dg);
int cnuda_dcn_v2_forward(const float* input, const float* weight, const float* bias,
                         const float* offset, const float* mask, float* output,
                         int B, int C, int H, int W, int Cout, int kh, int kw,
                         int sh, int sw, int ph, int pw, int dh, int dw, int dg,
                         void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_dcn_v2_backward(const float* input, const float* weight, const float* bias,
                          const float* offset, const float* mask, const float* grad_output,
                          float* grad_input, float* grad_offset, float* grad_mask,
                          float* grad_weight, float* grad_bias,
                          int B, int C, int H, int W, int Cout, int kh, int kw,
                          int sh, int sw, int ph, int pw, int dh, int dw, int dg,
                          void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* forward with a fused epilogue activation: output = act(dcn(...) + bias), act_slope < 0 none, 0 ReLU.  Used by
 * the BatchNorm-folded inference path (export.py), where the BatchNorm + ReLU of DeformConv (backends/dla.py:369-372)
 * live in the weights, the bias and this epilogue.  columns nullable as in forward_cols below. */
int cnuda_dcn_v2_forward_act(const float* input, const float* weight, const float* bias,
                             const float* offset, const float* mask, float* output, float* columns,
                             float act_slope,
                             int B, int C, int H, int W, int Cout, int kh, int kw,
                             int sh, int sw, int ph, int pw, int dh, int dw, int dg,
                             void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* forward (+ saved columns) that also leaves the BatchNorm statistics of the output, as cnuda_conv2d_forward_stats does:
 * DeformConv = DCN + BatchNorm + ReLU (backends/dla.py:351-372).  cnuda_dcn_v2_stats_block: 0 = none for this geometry,
 * else pixels per block (blocks are numbered image-major and never straddle images), *rows = rows per block. */
int cnuda_dcn_v2_stats_block(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                             int dh, int dw, int dg, int* rows);
/* stats_block / stats_rows: the layout the caller sized `stats` for (what cnuda_dcn_v2_stats_block answered).  The answer
 * depends on the kernel the call picks, and that on the offset regime (cnuda_dcn_set_offset_regime): a call whose own plan
 * disagrees with these two numbers fails instead of writing another layout into the caller's buffer. */
int cnuda_dcn_v2_forward_stats(const float* input, const float* weight, const float* bias, const float* offset,
                               const float* mask, float* output, float* columns, float* stats, int stats_block,
                               int stats_rows,
                               int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                               int dh, int dw, int dg, void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* Round 6 -- offsets and mask read straight out of `om` [B, 3*kh*kw, Ho, Wo], the output of DCN's own offset convolution
 * (libs/DCNv2/dcn_v2.py:118-122: o1, o2, mask = chunk(out, 3); offset = cat(o1, o2); mask = sigmoid(mask)): channels
 * 0 .. 2T-1 ARE the offsets, channels 2T .. 3T-1 the mask, ALREADY sigmoid (cnuda_conv2d_forward_rowsig applies it in the
 * convolution's epilogue).  backward_om writes ONE tensor grad_om of the same shape: the offsets' gradient and the gradient of
 * the mask's LOGIT (g * m * (1 - m), multiplied where the kernel stores) -- exactly what the offset convolution's backward
 * consumes.  Replaces the split / concatenate / sigmoid passes of the Python layer (32 launches of a benched step).
 * deformable_group == 1; columns / stats / accumulate_input as in forward_stats / backward_acc. */
int cnuda_dcn_v2_forward_om(const float* input, const float* weight, const float* bias, const float* om, float* output,
                            float* columns, float* stats, int stats_block, int stats_rows,
                            float act_slope /* < 0 none, 0 ReLU: the BatchNorm-folded inference path, as forward_act */,
                            int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                            int dh, int dw, int dg, void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_dcn_v2_backward_om(const float* input, const float* weight, const float* bias, const float* om,
                             const float* grad_output, const float* columns, float* grad_input, int accumulate_input,
                             float* grad_om, float* grad_weight, float* grad_bias,
                             int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                             int dh, int dw, int dg, void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* Same two operations with the sampled column buffer kept between them (the
 * product's autograd path): forward_cols stores
 * columns[B, kh*kw*C, Ho*Wo] (rows in (tap, channel) order, mask already applied;
 * deformable_group > 1: the groups' buffers [dg][B, kh*kw*C/dg, Ho*Wo] one behind the other, the same bytes)
 * as a side output of the implicit GEMM, backward_cols computes grad_weight as a
 * plain GEMM grad_output x columns^T instead of re-sampling the input.  With
 * columns == NULL both behave exactly like the entry points above.  The buffer
 * is what the reference materialises inside every call
 * (cuda/dcn_v2_cuda.cu:89-102); here it is written once and read once. */
int cnuda_dcn_v2_forward_cols(const float* input, const float* weight, const float* bias,
                              const float* offset, const float* mask, float* output, float* columns,
                              int B, int C, int H, int W, int Cout, int kh, int kw,
                              int sh, int sw, int ph, int pw, int dh, int dw, int dg,
                              void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_dcn_v2_backward_cols(const float* input, const float* weight, const float* bias,
                               const float* offset, const float* mask, const float* grad_output,
                               const float* columns,
                               float* grad_input, float* grad_offset, float* grad_mask,
                               float* grad_weight, float* grad_bias,
                               int B, int C, int H, int W, int Cout, int kh, int kw,
                               int sh, int sw, int ph, int pw, int dh, int dw, int dg,
                               void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* backward_cols with accumulate_input != 0: grad_input is NOT cleared first -- the data-gradient walks add into it (window
 * flushes and strays are atomics either way), so a caller that already holds another consumer's share of the input's
 * gradient there (the offset / mask convolution's input gradient: backends/dla.py:263-270, x feeds both) saves the clear and
 * autograd's sum.  accumulate_input == 0: exactly backward_cols. */
int cnuda_dcn_v2_backward_acc(const float* input, const float* weight, const float* bias,
                              const float* offset, const float* mask, const float* grad_output,
                              const float* columns,
                              float* grad_input, int accumulate_input, float* grad_offset, float* grad_mask,
                              float* grad_weight, float* grad_bias,
                              int B, int C, int H, int W, int Cout, int kh, int kw,
                              int sh, int sw, int ph, int pw, int dh, int dw, int dg,
                              void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * Deformable position-sensitive ROI pooling -- the other two functions of the native module
 * (libs/DCNv2/src/vision.cpp:6-7, cuda/dcn_v2_psroi_pooling_cuda.cu, float instantiation).
 *   input [B, channels, H, W], channels == output_dim * group_size^2;  rois [num_rois, 5] = (batch index, x1, y1, x2,
 *   y2), corners rounded half away from zero;  trans [num_rois, 2 * num_classes, part_size, part_size] (NULL and
 *   num_classes = 1 with no_trans != 0);  output, output_count [num_rois, output_dim, pooled_size, pooled_size], the
 *   count being the number of samples that fell inside the map (output 0 where it is 0).
 * pooled_size <= 64; output_dim % num_classes == 0.  The batch indices are read back to the host first (one stream
 * synchronisation per call): a ROI that names no image is CNUDA_ERR_INVALID_ARGUMENT, nothing is launched.
 * backward: grad_input [B, channels, H, W] is written (accumulate_input == 0) or added to (!= 0); grad_trans like
 * trans (untouched with no_trans).  Workspace (backward only): cnuda_dcn_v2_psroi_pooling_workspace_bytes.
 * No atomics: forward and backward are bit-stable from run to run (the reference's backward is not).
 * ---------------------------------------------------------------------- */
size_t cnuda_dcn_v2_psroi_pooling_workspace_bytes(int B, int num_rois, int output_dim, int pooled_size);
int cnuda_dcn_v2_psroi_pooling_forward(const float* input, const float* rois, const float* trans,
                                       float* output, float* output_count,
                                       int B, int channels, int H, int W, int num_rois, int no_trans,
                                       float spatial_scale, int output_dim, int group_size, int pooled_size,
                                       int part_size, int sample_per_part, float trans_std, int num_classes,
                                       cnuda_stream_t stream);
int cnuda_dcn_v2_psroi_pooling_backward(const float* grad_output, const float* input, const float* rois,
                                        const float* trans, const float* output_count,
                                        float* grad_input, int accumulate_input, float* grad_trans,
                                        int B, int channels, int H, int W, int num_rois, int no_trans,
                                        float spatial_scale, int output_dim, int group_size, int pooled_size,
                                        int part_size, int sample_per_part, float trans_std, int num_classes,
                                        void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * COCO evaluation (evaluation/coco.py): what pycocotools' computeIoU and evaluateImg do for one batch of images, with
 * the per-box masks of the rotated mode rasterised here instead of cv2.fillPoly + RLE.
 *   group: one (image, category), five ints {first detection, detections, first ground truth, ground truths, first
 *   pair}; detections of a group are consecutive and in descending score order, pair (d, g) is element
 *   first pair + d * ground truths + g of `iou`.  A group that does not fit num_det / num_gt / num_pairs is skipped.
 * cnuda_eval_box_spans: verts [num_boxes, 4, 2] integer (x, y) corners.  The mask of a box is the project's convex-fill
 *   rule (utils/image.py::_fill_convex_poly: 8-connected outline, then scanlines) clipped to H x W, held as one
 *   (left, right) span per image row in the workspace (cnuda_eval_workspace_bytes).  rows [num_boxes, 2]: first and
 *   last non-empty row (0, -1 for an empty mask); area [num_boxes]: pixel count.  H, W <= 8192.
 * cnuda_eval_iou_rotated: boxes [0, num_det) of that workspace are the detections, [num_det, num_det + num_gt) the
 *   ground truths; iou = |D and G| / (|D| + |G| - |D and G|) on pixel counts, 0 for an empty union.
 * cnuda_eval_iou_axis: boxes float32 (x, y, w, h); pycocotools' bbIou in double, 0 where width or height of the
 *   intersection is <= 0.  No fused multiply-add.
 * cnuda_eval_match: thresholds [num_thresholds <= 16] and area_ranges [4, 2] (lo, hi) are HOST arrays.  For every
 *   group and range: a ground truth is ignored when its area is < lo or > hi; detections in order take, among the
 *   ground truths not yet matched at that threshold with iou >= min(t, 1 - 1e-10), the non-ignored one of largest IoU
 *   (ties: the later one), else the ignored one by the same rule.  det_bits [num_det, 4]: bits 0..15 matched per
 *   threshold, bits 16..31 ignored per threshold (matched to an ignored ground truth, or unmatched with an area outside
 *   the range).  gt_ignore [num_gt, 4] bytes.  num_gt <= 16384 per call (one 32-bit word of LDS per ground truth).
 * cnuda_eval_match_flagged: cnuda_eval_match with gt_flags [num_gt] bytes: a ground truth whose flag is not 0 is
 *   ignored in every area range (COCOeval._prepare for keypoints: num_keypoints == 0), so a detection matched to it is
 *   ignored, not a false positive.  One kernel serves both entries; cnuda_eval_match passes no flags.
 * cnuda_eval_oks (evaluation/coco_keypoints.py): COCOeval.computeOks for every pair of every group, in float64 and in
 *   this order of operations.  det_kps [num_det, J, 2] and gt_kps [num_gt, J, 2] float32 (x, y); gt_vis [num_gt, J]
 *   bytes, COCO's v (a joint is labelled when v > 0); gt_area [num_gt] double; gt_box [num_gt, 4] float32 (x, y, w, h);
 *   sigmas [J] double, on the DEVICE; 1 <= J <= 64.  var_j = (2 sigma_j)^2; k1 = labelled joints of the ground truth.
 *   k1 > 0: dx_j = xd_j - xg_j, dy_j = yd_j - yg_j over the labelled joints.  k1 == 0: x0 = bx - bw, x1 = bx + 2 bw,
 *   y0 = by - bh, y1 = by + 2 bh; dx_j = max(0, x0 - xd_j) + max(0, xd_j - x1), dy_j likewise, over all J joints.
 *   e_j = (dx_j^2 + dy_j^2) / var_j / (area + 2^-52) / 2; oks = sum_j exp(-e_j) / n in ascending j, n = k1 or J.
 *   The same call writes det_area [num_det] double, (max x - min x) * (max y - min y) over a detection's J joints (the
 *   area COCO's loadRes gives a keypoint result), and gt_flags [num_gt] bytes, 1 where k1 == 0.  No fused multiply-add.
 * cnuda_eval_iou_quads: the rotated mode without masks.  quads [num_det + num_gt, 4, 2] float32 (x, y) vertices, the
 *   detections first; iou in the pair layout above is cnuda_quad_iou_pairs' exact polygon IoU with the detection as
 *   subject and the ground truth as clipper; area [num_det + num_gt] double: the polygon areas, written for every box
 *   whatever the groups say.  One launch, no workspace, no image size.
 * Integers and doubles only, no floating-point atomics: bit-stable.  Nothing synchronises the stream.
 * ---------------------------------------------------------------------- */
size_t cnuda_eval_workspace_bytes(int num_boxes, int H);
int cnuda_eval_box_spans(const int* verts, int num_boxes, int H, int W, int* rows, double* area,
                         void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_eval_iou_rotated(const int* groups, int num_groups, int num_det, int num_gt, long long num_pairs,
                           const int* rows, const double* area, int H, double* iou,
                           void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_eval_iou_axis(const float* det_boxes, const float* gt_boxes, const int* groups, int num_groups,
                        int num_det, int num_gt, long long num_pairs, double* iou, cnuda_stream_t stream);
int cnuda_eval_iou_quads(const float* quads, const int* groups, int num_groups, int num_det, int num_gt,
                         long long num_pairs, double* iou, double* area, cnuda_stream_t stream);
int cnuda_eval_match(const double* iou, const int* groups, int num_groups, const double* det_area,
                     const double* gt_area, int num_det, int num_gt, long long num_pairs,
                     const double* thresholds, int num_thresholds, const double* area_ranges,
                     unsigned* det_bits, unsigned char* gt_ignore, cnuda_stream_t stream);
int cnuda_eval_match_flagged(const double* iou, const int* groups, int num_groups, const double* det_area,
                             const double* gt_area, const unsigned char* gt_flags, int num_det, int num_gt,
                             long long num_pairs, const double* thresholds, int num_thresholds,
                             const double* area_ranges, unsigned* det_bits, unsigned char* gt_ignore,
                             cnuda_stream_t stream);
int cnuda_eval_oks(const float* det_kps, const float* gt_kps, const unsigned char* gt_vis, const double* gt_area,
                   const float* gt_box, const double* sigmas, int num_joints, const int* groups, int num_groups,
                   int num_det, int num_gt, long long num_pairs, double* oks, double* det_area,
                   unsigned char* gt_flags, cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * Dense convolution (groups 1, dilation 1) -- replaces torch.nn.Conv2d -> cuDNN
 * on the hot path: backends/dla.py:37-44,153-155,234-235,281-283,478-483 (DLA
 * trunk, roots, heads), libs/DCNv2/dcn_v2.py:104-110 (offset/mask conv),
 * backends/resnet.py:43-51 (heads), uda/adversarial_entropy_minimization.py:51-68
 * (discriminator).  weight is the state_dict layout [Cout, C, kh, kw].
 * forward: y = act(conv(x, w) + bias); bias may be NULL; act_slope < 0 -> no
 * activation, 0 -> ReLU, 0.2 -> LeakyReLU(0.2).  backward_weight writes
 * grad_weight (and grad_bias = channel sums of grad_y when non-NULL).
 * ---------------------------------------------------------------------- */
size_t cnuda_conv2d_workspace_bytes(int B, int C, int H, int W, int Cout, int kh, int kw,
                                    int sh, int sw, int ph, int pw);
int cnuda_conv2d_forward(const float* x, const float* weight, const float* bias, float* y,
                         int B, int C, int H, int W, int Cout, int kh, int kw,
                         int sh, int sw, int ph, int pw, float act_slope,
                         void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* forward with a residual input in the epilogue: y = act(conv(x, w) + bias + residual), residual shaped like y
 * (nullable).  The BatchNorm-folded inference path (export.py) runs a BasicBlock's second convolution, its
 * BatchNorm, the skip connection and the ReLU (backends/dla.py:48-62) as this one launch. */
int cnuda_conv2d_forward_res(const float* x, const float* weight, const float* bias, const float* residual, float* y,
                             int B, int C, int H, int W, int Cout, int kh, int kw,
                             int sh, int sw, int ph, int pw, float act_slope,
                             void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* forward with a sigmoid on the output channels >= sig_from (after the bias): the offset / mask convolution of a DCN layer
 * (libs/DCNv2/dcn_v2.py:104-122: channels 2T .. 3T-1 of its output are the modulation mask's logits) when the deformable
 * convolution reads offsets and mask out of this one tensor (cnuda_dcn_v2_forward_om).  cnuda_conv2d_rowsig_supported: 1 for
 * the geometries that have this epilogue (at most 32 output channels, C % 16 == 0, tensors below 2 GiB, f32 matrix mode). */
int cnuda_conv2d_rowsig_supported(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw);
int cnuda_conv2d_forward_rowsig(const float* x, const float* weight, const float* bias, float* y, int sig_from,
                                int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                                void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* A 1x1 convolution (stride 1, no padding) over the CHANNEL CONCATENATION of n = 2 .. 4 tensors xs[i] [B, cs[i], H, W]
 * without the concatenation: DLA's Root is conv(torch.cat(children, 1)) (backends/dla.py:150-168; 17 concatenated buffers per
 * forward pass of DLA-34 and their slices in the backward pass).  weight [Cout, sum cs, 1, 1] as for the concatenated tensor.
 * The GEMMs' K axis IS the concatenated channel axis: the gather switches source per 16-deep chunk, the input-gradient
 * epilogue stores every source's rows into its own tensor (+ adds[i] + add2s[i], nullable: the other consumers' shares of that
 * tensor's gradient, as cnuda_conv2d_backward_data_add), the weight gradient reads each 64-column group from its source.
 * stats: nullable, cnuda_conv2d_forward_stats' layout for the concatenated geometry (cnuda_conv2d_stats_block(B, sum cs, H, W,
 * Cout, 1, 1, 1, 1, 0, 0)).  cnuda_conv2d_cat_supported: every cs[i] % 64 == 0, H * W % 4 == 0, tensors below 2 GiB, the
 * concatenated geometry's plan without a K split, f32 matrix mode; elsewhere the caller concatenates.  Workspace:
 * cnuda_conv2d_workspace_bytes of the concatenated geometry. */
int cnuda_conv2d_cat_supported(const int* cs, int n, int B, int H, int W, int Cout);
int cnuda_conv2d_cat_forward(const float* const* xs, const int* cs, int n, const float* weight, const float* bias /* nullable */,
                             float* y, float* stats, float act_slope /* < 0: none; with stats: none */,
                             int B, int H, int W, int Cout, void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_conv2d_cat_backward_data(const float* grad_y, const float* weight, float* const* grad_xs, const float* const* adds,
                                   const float* const* add2s, const int* cs, int n, int B, int H, int W, int Cout,
                                   void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_conv2d_cat_backward_weight(const float* const* xs, const int* cs, int n, const float* grad_y, float* grad_weight,
                                     int B, int H, int W, int Cout, void* workspace, size_t workspace_bytes,
                                     cnuda_stream_t stream);
/* forward whose output channels are interleaved in quads: y[B][Cout / 4][Ho * Wo][4] (channel m of pixel p at
 * ((m >> 2) * Ho*Wo + p) * 4 + (m & 3)); no bias, no activation.  The layout of the DCN column gradient (round 6): the
 * gradient walk of cnuda_dcn_v2_backward reads the four channels of a (pixel, tap) with one 16-byte load.  Replaces nothing
 * of the reference's (its dcn_v2_cuda.cu:262-275 GEMM writes [kh*kw*C][Ho*Wo] rows); internal to the backward, exported so
 * that the layout has a value test of its own.  cnuda_conv2d_rowquads_supported: Cout % 4 == 0, C % 16 == 0, tensors below
 * 2 GiB, no K split in the plan. */
int cnuda_conv2d_rowquads_supported(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw);
int cnuda_conv2d_forward_rowquads(const float* x, const float* weight, float* y,
                                  int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                                  void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* forward that also leaves the statistics a train-mode BatchNorm of y needs (the layer behind almost every convolution of
 * DLA-34, backends/dla.py:37-62,150-168: the reference's cuDNN BatchNorm re-reads y for them; here the GEMM's epilogue sums
 * what it stores).  stats: [blocks][rows][2] floats = (sum, sum of squares) of y over one block of `cnuda_conv2d_stats_block`
 * consecutive pixels of the flattened (image, pixel) axis, per output channel (row); blocks = ceil(B*Ho*Wo / 128) * (128 /
 * block pixels).  cnuda_conv2d_stats_block returns 0 where this geometry's kernel cannot give them (then pass stats =
 * NULL and use cnuda_bn_train_forward), else the block size, and *rows.  Needs residual == NULL and act_slope < 0.
 * cnuda_bn_train_forward_stats (below) consumes them. */
int cnuda_conv2d_stats_block(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int* rows,
                             int* blocks_per_image /* > 0: blocks are pieces of output rows, this many per image (the 3- / 16-
                                                      channel layers' kernels) and `stats` holds B * blocks_per_image of them */);
int cnuda_conv2d_forward_stats(const float* x, const float* weight, const float* bias, const float* residual, float* y,
                               float* stats, int B, int C, int H, int W, int Cout, int kh, int kw,
                               int sh, int sw, int ph, int pw, float act_slope,
                               void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_conv2d_backward_data(const float* grad_y, const float* weight, float* grad_x,
                               int B, int C, int H, int W, int Cout, int kh, int kw,
                               int sh, int sw, int ph, int pw,
                               void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* Apply on load: x is the output of a convolution whose train-mode BatchNorm + ReLU has NOT been applied
 * (cnuda_bn_train_forward_stats with y == NULL left save_mean / save_invstd, [groups][C]); the kernel computes
 * max(x * (invstd * gamma) + (beta - mean * invstd * gamma), 0) while it stages x, per statistics group of imgs_per_group
 * images -- bit-identical to convolving the materialised activation, one pass over it less in each direction.  Replaces
 * the pass of reference backends/dla.py:19,40 (nn.BatchNorm2d + ReLU between two convolutions) for the geometries
 * cnuda_conv2d_norm_input_supported() returns 1 for; the other arguments as cnuda_conv2d_forward_stats /
 * cnuda_conv2d_backward_weight. */
int cnuda_conv2d_norm_input_supported(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw);
int cnuda_conv2d_forward_norm_input(const float* x, const float* mean, const float* invstd, const float* gamma,
                                    const float* beta, int imgs_per_group, const float* weight, const float* bias, float* y,
                                    float* stats, int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph,
                                    int pw, float act_slope, void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_conv2d_backward_weight_norm_input(const float* x, const float* mean, const float* invstd, const float* gamma,
                                            const float* beta, int imgs_per_group, const float* grad_y, float* grad_weight,
                                            float* grad_bias, int B, int C, int H, int W, int Cout, int kh, int kw, int sh,
                                            int sw, int ph, int pw, void* workspace, size_t workspace_bytes,
                                            cnuda_stream_t stream);
/* grad_x = input gradient + addend + addend2 (both nullable, shaped like grad_x, either may BE grad_x): where a tensor
 * feeds a convolution and something else (a skip connection, a concatenation, a DCN's sampling), the other consumers'
 * shares of its gradient are summed in the epilogue of this one instead of by passes of their own (what autograd's
 * accumulation does in the reference: torch's engine, one at::add per extra consumer; hip_runtime.fanout). */
int cnuda_conv2d_backward_data_add(const float* grad_y, const float* weight, const float* addend, const float* addend2,
                                   float* grad_x,
                                   int B, int C, int H, int W, int Cout, int kh, int kw,
                                   int sh, int sw, int ph, int pw,
                                   void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_conv2d_backward_weight(const float* x, const float* grad_y, float* grad_weight, float* grad_bias,
                                 int B, int C, int H, int W, int Cout, int kh, int kw,
                                 int sh, int sw, int ph, int pw,
                                 void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * BatchNorm2d fused with the residual add and ReLU that follow it in DLA-34
 * (backends/dla.py:48-62,150-168,277-287,351-372; nn.BatchNorm2d(momentum=0.1)).
 * x, y, residual: [B, C, HW].  residual may be NULL; relu: 0 none, 1 max(.,0), 2 ReLU6 = min(max(.,0),6)
 * (gradient strictly inside (0,6), torch's hardtanh backward).
 * train_forward updates running_mean/var in place (unbiased variance, may be
 * NULL) and saves mean / invstd for backward.  backward: grad_y is the gradient
 * w.r.t. y (post-activation); y is needed only when relu != 0; grad_residual
 * (nullable) receives the gradient flowing into the residual branch.
 * ---------------------------------------------------------------------- */
size_t cnuda_bn_workspace_bytes(int B, int C, long long HW);
/* The run-time form that train_forward / backward take for this geometry (one kernel body serves all of them, so the
 * kernel names cannot tell): per_plane = chunks one (image, channel) plane is cut into for the statistics,
 * images_per_workgroup = images of one channel that one workgroup takes (> 1 only with per_plane == 1), partials = fp64
 * partial sums per channel (B / images_per_workgroup * per_plane), apply_splits = workgroups per plane (gridDim.y) of
 * the two apply passes.  Every result pointer is nullable.  Answered by the entry points' own planning code; no GPU
 * needed.  -1 (cnuda_last_error) for an empty tensor or a batch that `groups` does not divide. */
int cnuda_bn_plan(int B, int C, long long HW, int groups, int* per_plane, int* images_per_workgroup, int* partials,
                  int* apply_splits);
int cnuda_bn_train_forward(const float* x, const float* gamma, const float* beta, const float* residual,
                           float* y, float* save_mean, float* save_invstd,
                           float* running_mean, float* running_var,
                           long long* num_batches_tracked /* nullable; += 1 like nn.BatchNorm2d.forward */,
                           float momentum, float eps, int relu,
                           int B, int C, long long HW,
                           int groups /* statistics groups: images [g*B/groups, (g+1)*B/groups) are normalised by their
                                         own batch statistics (save_mean / save_invstd are [groups][C]) and the running
                                         statistics take one momentum update per group, in group order -- one call on
                                         the concatenated source | target batch equals the reference's two forward
                                         calls (uda/entropy_minimization.py:18-19) */,
                           void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* train_forward with sum(x) / sum(x^2) supplied by the kernel that produced x (cnuda_conv2d_forward_stats,
 * cnuda_dcn_v2_forward_stats): no statistics pass over x.  stats [blocks][rows][2], blocks numbered image-major; group g =
 * blocks [g, g + 1) * blocks_per_group (the caller checks that a statistics group is whole blocks). */
int cnuda_bn_train_forward_stats(const float* x, const float* stats, long long blocks_per_group, int rows, const float* gamma,
                                 const float* beta, const float* residual, float* y, float* save_mean, float* save_invstd,
                                 float* running_mean, float* running_var, long long* num_batches_tracked,
                                 float momentum, float eps, int relu, int B, int C, long long HW, int groups,
                                 void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_bn_eval_forward(const float* x, const float* gamma, const float* beta,
                          const float* running_mean, const float* running_var, const float* residual,
                          float* y, float eps, int relu, int B, int C, long long HW, cnuda_stream_t stream);
int cnuda_bn_backward(const float* grad_y, const float* x, const float* y, const float* gamma,
                      const float* beta /* nullable.  Given (only without a residual): the activation's gate is
                                           recomputed from x with the forward's own multiply and add instead of read
                                           from y -- one tensor less per pass; y may then be NULL */,
                      const float* save_mean, const float* save_invstd,
                      float* grad_x, float* grad_residual, float* grad_gamma, float* grad_beta,
                      int relu, int B, int C, long long HW, int groups,
                      void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * Spatial / elementwise pieces of the DLA graph.
 *   maxpool2d: window k, stride k, no padding  (nn.MaxPool2d(stride, stride), dla.py:202-203)
 *   dwconvt2d: depthwise ConvTranspose2d, weight [C,1,k,k], stride s, padding p, no bias
 *              (IDAUp.up, dla.py:385-388: k = 2f, s = f, p = f/2); grad_x / grad_w nullable
 *   add, act_backward (gx = gy * (y > 0 ? 1 : slope)), copy_channels (concat / slice),
 *   split_offset_mask: DCN.forward's chunk/cat/sigmoid (libs/DCNv2/dcn_v2.py:119-122)
 * ---------------------------------------------------------------------- */
int cnuda_maxpool2d_forward(const float* x, float* y, int B, int C, int H, int W, int k, cnuda_stream_t stream);
int cnuda_maxpool2d_backward(const float* x, const float* grad_y, float* grad_x,
                             int B, int C, int H, int W, int k, cnuda_stream_t stream);
/* ... with accumulate != 0: grad_x already holds another consumer's share of x's gradient (hip_runtime.fanout: a level input
 * that feeds the pooling shortcut and a strided convolution, backends/dla.py:199-203) and only the arg-max cell of every window
 * is touched (+= grad_y). */
int cnuda_maxpool2d_backward_acc(const float* x, const float* grad_y, float* grad_x, int accumulate, int B, int C, int H, int W,
                                 int k, cnuda_stream_t stream);
/* general window (kernel k, stride s, padding p with -inf, floor mode): torchvision's ResNet stem pool
 * nn.MaxPool2d(3, 2, 1), kept inside `base` by backends/resnet.py:27-30.  Backward is a deterministic gather. */
int cnuda_maxpool2d_window_forward(const float* x, float* y, int B, int C, int H, int W, int k, int s, int p,
                                   cnuda_stream_t stream);
int cnuda_maxpool2d_window_backward(const float* x, const float* grad_y, float* grad_x,
                                    int B, int C, int H, int W, int k, int s, int p, cnuda_stream_t stream);
int cnuda_dwconvt2d_forward(const float* x, const float* w, float* y,
                            int B, int C, int H, int W, int k, int s, int p, cnuda_stream_t stream);
/* y = dwconvt2d(x, w) + skip with skip of the output's shape (nullable): IDAUp's `up(project(x)) + layers[i-1]`
 * (dla.py:400-401) in one pass over the upsampled map, rounded as the separate add would round */
int cnuda_dwconvt2d_add_forward(const float* x, const float* w, const float* skip, float* y,
                                int B, int C, int H, int W, int k, int s, int p, cnuda_stream_t stream);
size_t cnuda_dwconvt2d_workspace_bytes(int B, int C, int k);   /* per-image partial weight gradients */
int cnuda_dwconvt2d_backward(const float* x, const float* w, const float* grad_y, float* grad_x, float* grad_w,
                             int B, int C, int H, int W, int k, int s, int p,
                             void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* Depthwise convolution, weight [C,1,k,k] (k = 3 or 5), no bias -- torchvision MobileNetV2's
 * `nn.Conv2d(hidden, hidden, 3, stride, 1, groups=hidden, bias=False)` inside backends/mobilenetv2.py:31-36's hub
 * trunk.  Any stride s >= 1 and padding p >= 0 on every side; the output is (H + 2p - k) / s + 1 rows (floor), likewise
 * for W.  backward writes grad_x and/or grad_w (either may be NULL); grad_w needs the workspace.  These calls are
 * cnuda_dwconv2d_same_* below with pad_top = pad_left = p and that output size, on the same kernels with the same
 * rounding, without that pair's limits on stride and padding. */
size_t cnuda_dwconv2d_workspace_bytes(int B, int C, int k);
int cnuda_dwconv2d_forward(const float* x, const float* w, float* y, int B, int C, int H, int W, int k, int s, int p,
                           cnuda_stream_t stream);
int cnuda_dwconv2d_backward(const float* x, const float* w, const float* grad_y, float* grad_x, float* grad_w,
                            int B, int C, int H, int W, int k, int s, int p,
                            void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_add(const float* a, const float* b, float* out, long long n, cnuda_stream_t stream);
int cnuda_act_backward(const float* grad_y, const float* y, float* grad_x, long long n, float slope,
                       cnuda_stream_t stream);
/* grad_hidden = act'(hidden) * conv1x1_input_gradient(grad_y, weight): the last layer of a detection head
 * (nn.Conv2d(head_conv, classes, 1), dla.py:474-483) has 1..8 output channels, so its input gradient is one pass over
 * the hidden map fused with the backward of the ReLU in front of it.  weight [Co, Ch] (the 1x1 kernel), hidden /
 * grad_hidden [B, Ch, HW] (HW % 4 == 0), grad_y [B, Co, HW]; channels summed in increasing order. */
int cnuda_conv1x1_backward_data_act(const float* grad_y, const float* weight, const float* hidden, float* grad_hidden,
                                    int B, int Co, int Ch, long long HW, float slope, cnuda_stream_t stream);
/* The whole backward of a detection head -- conv(C -> Ch, kh x kw, stride 1, "same" padding) + act + conv1x1(Ch -> Co) --
 * for a grad_y [B, Co, HW] that is zero outside the cells ind[b][m] with mask[b][m] != 0 (the gradient of the gather +
 * masked-L1 loss, cnuda_reg_l1_backward).  The active rows (mask set, 0 <= ind < HW, first of the rows of its image with that
 * ind: the dense map already holds the sum of duplicates) are gathered into compact [channels][R] matrices, R = B * M
 * rounded up to 4, inactive rows zero; the parameter gradients and the patch gradients are 1x1 convolution calls over
 * them (cnuda_conv2d_backward_weight / _backward_data: fixed-order sums), the patch gradients are added to grad_x by plain
 * read-add-write -- rows with no other row within kh - 1 pixels in parallel, the others of an image in row order -- so
 * every result is run-to-run bit-reproducible.  x, hidden: the B images the head saw; grad_x [B, C, H, W] is ADDED to (nullable); grad_w1 [Ch, C, kh, kw],
 * grad_b1 [Ch], grad_w2 [Co, Ch], grad_b2 [Co] are written (each nullable).  Values: those of cnuda_conv2d_backward_weight,
 * cnuda_conv1x1_backward_data_act and cnuda_conv2d_backward_data on the dense map up to the order of the sums.
 * _supported: stride 1, 1 <= Co <= 8, odd kh == kw <= 7 with ph == pw == (kh - 1) / 2, M <= 4096, B * M < 2^20. */
int cnuda_head_backward_sparse_supported(int B, int M, int C, int H, int W, int Ch, int Co, int kh, int kw, int sh, int sw,
                                         int ph, int pw);
size_t cnuda_head_backward_sparse_workspace_bytes(int B, int M, int C, int H, int W, int Ch, int Co, int kh, int kw);
int cnuda_head_backward_sparse(const float* grad_y, const long long* ind, const unsigned char* mask, const float* x,
                               const float* hidden, const float* w1, const float* w2, float* grad_x, float* grad_w1,
                               float* grad_b1, float* grad_w2, float* grad_b2, int B, int M, int C, int H, int W, int Ch,
                               int Co, int kh, int kw, float slope, void* workspace, size_t workspace_bytes,
                               cnuda_stream_t stream);
int cnuda_copy_channels(const float* src, float* dst, int B, int Cn, long long HW,
                        int Csrc, int src_off, int Cdst, int dst_off, cnuda_stream_t stream);
int cnuda_split_offset_mask(const float* om, float* offset, float* mask, int B, int taps, long long HW,
                            cnuda_stream_t stream);
int cnuda_split_offset_mask_backward(const float* grad_offset, const float* grad_mask, const float* mask,
                                     float* grad_om, int B, int taps, long long HW, cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * Losses.  Scalars live in device memory (no host sync; the reference's
 * `if num_pos == 0` host branch, losses/centernet.py:91, is taken on device).
 * `upstream` is a device pointer to the scalar gradient of the loss value.
 *   focal   : losses/centernet.py:69-95 on prob = clamp(sigmoid(logits)) (utils/tensor.py:5-7);
 *             out2 = {loss, num_pos}; prob receives the clamped probabilities (Q1)
 *   reg_l1  : losses/centernet.py:98-133 (ch 2, or 3 = rotated) and :192-223 (periodic != 0);
 *             masks `target` in place and, for the rotated non-periodic angle, replaces it by its
 *             sigmoid, as the reference does (Q2); out2 = {loss, mask.sum()+1e-4}
 *   softmax_loss kind 0: losses/entropy.py:10-28; kind 1: losses/max_square.py:6-14
 *   entropy_map: utils/image.py:121-124;  bce_const: losses/advent.py:10-18
 * ---------------------------------------------------------------------- */
size_t cnuda_loss_workspace_bytes(void);
int cnuda_focal_loss_forward(const float* logits, const float* gt, float* prob, float* out2, long long n,
                             float weight, void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_focal_loss_backward(const float* logits, const float* gt, const float* out2, const float* upstream,
                              float* grad_logits, long long n, float weight, cnuda_stream_t stream);
int cnuda_reg_l1_forward(const float* feat, const uint8_t* mask, const int64_t* ind, float* target, float* out2,
                         int B, int M, int ch, long long HW, int periodic, float weight, float angle_weight,
                         cnuda_stream_t stream);
int cnuda_reg_l1_backward(const float* feat, const uint8_t* mask, const int64_t* ind, const float* target,
                          const float* out2, const float* upstream, float* grad_feat,
                          int B, int M, int ch, long long HW, int periodic, float weight, float angle_weight,
                          cnuda_stream_t stream);
/* KPSL1Loss (losses/centernet.py:136-189): feat [B,2J,HW], mask [B,M,2J] (kp_reg_mask, datasets/coco.py:183,226-227),
 * target [B,M,2J] masked in place; pairs [n_pairs][2] int32 = kps_weight_indices (NULL / 0: no distance term);
 * use_l1 selects the L1 pair distance, else sqrt(|.|^2 + 1e4) (:175-179); out2 = {loss, mask.sum() + 1e-4}. */
int cnuda_kps_l1_forward(const float* feat, const uint8_t* mask, const int64_t* ind, float* target,
                         const int32_t* pairs, float* out2, int B, int M, int J, long long HW, int n_pairs,
                         int use_l1, float weight, float distance_weight, cnuda_stream_t stream);
int cnuda_kps_l1_backward(const float* feat, const uint8_t* mask, const int64_t* ind, const float* target,
                          const int32_t* pairs, const float* out2, const float* upstream, float* grad_feat,
                          int B, int M, int J, long long HW, int n_pairs, int use_l1, float weight,
                          float distance_weight, cnuda_stream_t stream);
int cnuda_softmax_loss_forward(const float* logits, float* out1, int B, int C, long long HW, int kind,
                               void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_softmax_loss_backward(const float* logits, const float* upstream, float* grad_logits,
                                int B, int C, long long HW, int kind, cnuda_stream_t stream);
int cnuda_entropy_map_forward(const float* logits, float* out, int B, int C, long long HW, cnuda_stream_t stream);
int cnuda_entropy_map_backward(const float* logits, const float* grad_out, float* grad_logits,
                               int B, int C, long long HW, cnuda_stream_t stream);
/* eta-weighted EntropyLoss (losses/entropy.py:17-22, used by the FDA plugin): e = -sum_c v log2(v + 1e-30) / log2(C)
 * per pixel of softmax(logits) over C, out1 = mean over B x HW of (e^2 + 1e-30)^eta.  Same workspace as the other losses. */
int cnuda_entropy_eta_loss_forward(const float* logits, float* out1, int B, int C, long long HW, float eta,
                                   void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_entropy_eta_loss_backward(const float* logits, const float* upstream, float* grad_logits,
                                    int B, int C, long long HW, float eta, cnuda_stream_t stream);
/* Image-wise class-balanced max-squares (Chen, Xue, Cai, ICCV 2019; the reference ships only the plain form).
 *   a[b,p] = argmax_c logits[b,c,p], the lowest channel on a tie;  hist[b,c] = #{p : a[b,p] == c}  (int32, sums to HW)
 *   w[b,c] = 1 / max(hist[b,c]^ratio * HW^(1-ratio), 1)  (float32);  out1 = -sum_{b,c,p} v^2 w[b,a[b,p]] / (2 B C),
 *   v = softmax over C: the published form divided by 2 as MaxSquareLoss is, so ratio = 0 gives MaxSquareLoss.
 * argmax_histogram clears `hist` itself; forward writes the weights [B*C] that backward reads.  C <= 1024 (the
 * workgroup's LDS table), 0 <= ratio <= 1.  No call synchronises; integer counts and fp64 sums: the same bits every run. */
int cnuda_argmax_histogram(const float* logits, int32_t* hist, int B, int C, long long HW, cnuda_stream_t stream);
int cnuda_iw_max_square_forward(const float* logits, const int32_t* hist, float ratio, float* weights_out, float* out1,
                                int B, int C, long long HW, void* workspace, size_t workspace_bytes,
                                cnuda_stream_t stream);
int cnuda_iw_max_square_backward(const float* logits, const float* weights, const float* upstream, float* grad_logits,
                                 int B, int C, long long HW, cnuda_stream_t stream);
/* Multi-level self-produced guidance (the same paper's third part; neither in the reference).  high, low [B,C,HW]: the
 * logits of the final and of the low-level heat map.  p = softmax_C(high), q = softmax_C(low), e = (p + q) / 2,
 * a = argmax_c e (the lowest channel on a tie); a pixel is guided when max_c e > threshold, 0 <= threshold < 1.
 *   labels[b,p] = a, or -1 where unguided (int32 [B,HW]);   N = number of guided pixels of the whole batch
 *   out2 = {sum_{guided} (logsumexp_c low - low[a]) / max(N, 1), N}: finite for any logits, {0, 0} without a guided pixel.
 * backward: grad_low = upstream * guided * (q_c - [c == a]) / max(N, 1), every element written (plain zeros where
 * unguided); `high` has no gradient.  No call synchronises; fp64 sums in a fixed order, no float atomics: the same bits
 * every run. */
int cnuda_guidance_forward(const float* high, const float* low, float threshold, int32_t* labels, float* out2, int B,
                           int C, long long HW, void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
int cnuda_guidance_backward(const float* low, const int32_t* labels, const float* out2, const float* upstream,
                            float* grad_low, int B, int C, long long HW, cnuda_stream_t stream);
int cnuda_bce_const_forward(const float* logits, float label, float* out1, long long n, cnuda_stream_t stream);
int cnuda_bce_const_backward(const float* logits, float label, const float* upstream, float* grad_logits,
                             long long n, cnuda_stream_t stream);
/* x <- sigmoid(x) in place, y = clamp(x, 1e-4, 1-1e-4)  (utils/tensor.py:5-7) */
int cnuda_sigmoid_clamp_(float* x, float* y, long long n, cnuda_stream_t stream);
/* feat [B,ch,HW], ind [B,M] -> out [B,M,ch]  (utils/tensor.py:10-25) */
int cnuda_gather_feat(const float* feat, const int64_t* ind, float* out, int B, int M, int ch, long long HW,
                      cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * EfficientNet MBConv block (backends/efficientnet.py; csrc/mbconv.hip, the depthwise convolution csrc/spatial.hip).
 * fp32, caller's stream, no float atomics: every reduction has a fixed order and two runs give the same bits.
 *
 * Depthwise convolution with TensorFlow "SAME" padding, weight [C,1,k,k] (k = 3 or 5, stride 1 or 2), no bias:
 *   y[b,c,oy,ox] = sum_{r,t} w[c,r,t] * x[b,c, oy*s - pad_top + r, ox*s - pad_left + t], zero outside the map.
 * The bottom / right padding is implied by the output size, (Ho-1)*s + k - pad_top - H (and likewise for W); it must
 * lie in [0, k) like pad_top / pad_left.  backward writes grad_x and/or grad_w (either may be NULL); grad_w needs the
 * workspace (per-image partial sums, added in image order).  The kernels are those of cnuda_dwconv2d_* above.
 * ---------------------------------------------------------------------- */
size_t cnuda_dwconv2d_same_workspace_bytes(int B, int C, int k);
int cnuda_dwconv2d_same_forward(const float* x, const float* w, float* y, int B, int C, int H, int W, int k, int s,
                                int pad_top, int pad_left, int Ho, int Wo, cnuda_stream_t stream);
int cnuda_dwconv2d_same_backward(const float* x, const float* w, const float* grad_y, float* grad_x, float* grad_w,
                                 int B, int C, int H, int W, int k, int s, int pad_top, int pad_left, int Ho, int Wo,
                                 void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* y = x * sigmoid(x);  grad_x = grad_y * (s + x*s*(1-s)), s = sigmoid(x), recomputed from x */
int cnuda_swish_forward(const float* x, float* y, long long n, cnuda_stream_t stream);
int cnuda_swish_backward(const float* grad_y, const float* x, float* grad_x, long long n, cnuda_stream_t stream);
/* Squeeze-and-excite: pool[b,c] = mean_hw x;  hpre = W1 pool + b1 (W1 [Cse,C]);  gate = sigmoid(W2 swish(hpre) + b2)
 * (W2 [C,Cse]);  y = x * gate[b,c].  One workgroup per image computes the gate with pool and the hidden vector in LDS
 * ((C + Cse) * 4 bytes <= 60 KiB).  pool [B,C], hpre [B,Cse], gate [B,C] are outputs the backward takes back:
 *   dg = sum_hw grad_y * x;  grad_x = grad_y * gate + dpool / HW;  grad_w1 / grad_b1 / grad_w2 / grad_b2 summed over the
 *   images in increasing order (each nullable).  Workspace: cnuda_se_workspace_bytes. */
size_t cnuda_se_workspace_bytes(int B, int C, int Cse);
int cnuda_se_forward(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y,
                     float* pool, float* hpre, float* gate, int B, int C, int Cse, long long HW, cnuda_stream_t stream);
int cnuda_se_backward(const float* x, const float* grad_y, const float* w1, const float* w2, const float* pool,
                      const float* hpre, const float* gate, float* grad_x, float* grad_w1, float* grad_b1,
                      float* grad_w2, float* grad_b2, int B, int C, int Cse, long long HW,
                      void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* Drop-connect + residual: y[b,i] = x[b,i] * mask[b] + residual[b,i], mask [B] from the caller.  residual NULL:
 * y = x * mask[b], which also is the backward (grad_x = grad_y * mask[b]; grad_residual = grad_y). */
int cnuda_drop_connect_add(const float* x, const float* mask, const float* residual, float* y, int B,
                           long long per_image, cnuda_stream_t stream);
/* y [planes, H+pad_bottom, W+pad_right] = x [planes,H,W] in the top-left corner, zeros elsewhere: the SAME padding of
 * the dense stride-2 stem, so that the implicit-GEMM loaders keep their symmetric padding.  No backward. */
int cnuda_pad_right_bottom(const float* x, float* y, long long planes, int H, int W, int pad_bottom, int pad_right,
                           cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * Fourier domain adaptation (utils/image.py:137-230, FDA_source_to_target): out = irfft2 of the source's half
 * spectrum (columns 0 .. W/2) whose amplitude is replaced by the target's where use_target_amp[ky][kx] != 0
 * (a bin with |S| = 0 becomes (|T|, 0)); the DC and Nyquist columns contribute their real part only.
 *   src, trg, out [B,C,H,W] f32;  use_target_amp [H][W/2+1] u8, shared by every image and channel.
 * H, W <= 4096.  Workspace: cnuda_fda_workspace_bytes (the two half spectra, 2*B*C*H*(W/2+1) complex fp32).
 * Deterministic (no atomics).  Not differentiable (the reference never back-propagates through it).
 * ---------------------------------------------------------------------- */
size_t cnuda_fda_workspace_bytes(int B, int C, int H, int W);
int cnuda_fda_source_to_target(const float* src, const float* trg, const uint8_t* use_target_amp, float* out,
                               int B, int C, int H, int W, void* workspace, size_t workspace_bytes,
                               cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * Optimizer -- torch.optim.Adam arithmetic (train.py:88-90) over a flat arena.
 * step is the 1-based step count used for bias correction.
 * ---------------------------------------------------------------------- */
int cnuda_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    cnuda_stream_t stream);
/* The other update rules of torch.optim over a flat range of the arena (csrc/optim.hip): torch's single-tensor
 * arithmetic in torch's order of operations, every operand n fp32.  A range begins and ends on an arena slot boundary:
 * every pointer must be 16-byte aligned and n a multiple of 4 (checked).  Optional operands are NULL exactly when the
 * rule does not use them.  Hyper-parameters are doubles: the derived constants (1 - dampening, 1 - lr*wd, lr / bias
 * correction, ...) are formed in double, as torch forms them in Python floats, and rounded to fp32 once.  flags are 0 / 1.
 * Elements whose gradient and state are all zero (the arena's alignment gaps) stay finite for every eps, eps = 0
 * included: a zero numerator gives a zero quotient.
 *   sgd:     momentum_buffer NULL <=> momentum == 0;  first = 1: this is the range's first update (buf = g);
 *            nesterov needs momentum > 0 and dampening == 0.
 *   adamw:   Adam family beyond plain Adam.  decoupled = 1: p *= 1 - lr*wd (AdamW), 0: g += wd*p (Adam);
 *            max_exp_avg_sq non-NULL: amsgrad;  step: 1-based count of updates of this range (bias correction).
 *   rmsprop: grad_avg non-NULL: centered;  momentum_buffer NULL <=> momentum == 0. */
int cnuda_sgd_step(float* param, const float* grad, float* momentum_buffer, long long n, double lr, double momentum,
                   double dampening, double weight_decay, int nesterov, int maximize, int first, cnuda_stream_t stream);
int cnuda_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                     long long n, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int decoupled, int maximize, int step, cnuda_stream_t stream);
int cnuda_rmsprop_step(float* param, const float* grad, float* square_avg, float* grad_avg, float* momentum_buffer,
                       long long n, double lr, double alpha, double eps, double weight_decay, double momentum,
                       int maximize, cnuda_stream_t stream);

/* ------------------------------------------------------------------------
 * Target encoding for a batch (the step right before the hot path):
 * datasets/coco.py:191-221 (per-object loop: clip, gaussian radius, centre, ind / wh / reg / reg_mask /
 * gt_dets / gt_areas) and utils/image.py:8-57 (gaussian_radius, draw_umich_gaussian), all images in one launch.
 *   boxes [B,M,4] double (x1,y1,x2,y2 in output-map pixels, after augmentation / clip_out_of_image),
 *   classes [B,M] int32, counts [B] int32 (objects per image, <= M).  Every output is fully overwritten
 *   (zeros where the reference leaves np.zeros): hm [B,C,H,W] f32, reg_mask [B,M] u8, ind [B,M] i64,
 *   wh / reg [B,M,2] f32, gt_dets [B,M,6] f32, gt_areas [B,M] f32 (= w*h: annotations without "area").
 * cnuda_encode_targets is cnuda_encode_targets_modes below with boxes alone (corners, keypoints, visibility, areas,
 * kps, gt_kps, kp_reg_mask NULL, J = 0): the same checks, the same kernel; errors carry that call's name.
 * ---------------------------------------------------------------------- */
int cnuda_encode_targets(const double* boxes, const int* classes, const int* counts,
                         float* hm, unsigned char* reg_mask, long long* ind, float* wh, float* reg,
                         float* gt_dets, float* gt_areas,
                         int B, int C, int H, int W, int M, cnuda_stream_t stream);
/* The encoder with every mode of the dataset's loop (datasets/coco.py:176-184,217-233 keypoints and "area"; 303-376
 * rotated boxes), one workgroup per (image, slot).  Exactly one of boxes / corners is non-NULL.
 *   corners [B,M,4,2] double: the four corner points in output-map pixels.  Each is clipped to [0,W-1] x [0,H-1] and
 *     rounded to float32; the object becomes the least-area enclosing rectangle with a side along an edge of the
 *     points' convex hull (what the reference asks of cv2.minAreaRect), in double from the float32 points, then
 *     utils/box.py's normalisation on float32 values: w the short side, h the long one (w == h: h += 1), angle the
 *     direction of the short side in degrees (y down, the convention of rotate_bbox) folded into [-90, 90).  Fewer
 *     than three hull vertices or a zero extent: the slot stays zero (the reference's `continue`).  Then wh is
 *     [B,M,3] (w, h, angle) and gt_dets [B,M,7] (cx, cy, w, h, angle, 1, class); with boxes they are [B,M,2] / [B,M,6].
 *   keypoints [B,M,J,2] double, visibility [B,M,J] int32 (COCO's v), kps [B,M,2J] f32 (offsets from the integer
 *     centre), gt_kps [B,M,J,2] f32, kp_reg_mask [B,M,2J] u8 (v == 2 and 0 <= x < W and 0 <= y < W: the reference
 *     tests y against the width): all five non-NULL when J > 0, all NULL when J == 0.  Written for valid slots only.
 *   areas [B,M] f32 or NULL: the annotation's "area"; NaN (or NULL) = absent, gt_areas falls back to w*h.
 *   counts is clamped to M.  Every output is fully overwritten. */
int cnuda_encode_targets_modes(const double* boxes, const double* corners, const int* classes, const int* counts,
                               const double* keypoints, const int* visibility, const float* areas,
                               float* hm, unsigned char* reg_mask, long long* ind, float* wh, float* reg,
                               float* gt_dets, float* gt_areas, float* kps, float* gt_kps,
                               unsigned char* kp_reg_mask,
                               int B, int C, int H, int W, int M, int J, cnuda_stream_t stream);
/* Input normalisation (datasets/coco.py:160-162, 105-109): images [B,H,W,3] uint8 (4-byte aligned) ->
 * out [B,3,H,W] f32 (16-byte aligned), out = (float(u8) / 255 - mean_c) / std_c, each step one IEEE float32
 * operation: bit-identical to the numpy expression. */
int cnuda_prepare_input(const unsigned char* images, float* out, int B, int H, int W,
                        float mean0, float mean1, float mean2, float std0, float std1, float std2,
                        cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Augmentation and resizing (the reference's imgaug chain, datasets/coco.py:140-158, restated geometrically: DESIGN.md,
 * "Augmentation on the device").  The draws and the matrices come from the host; these calls apply them.
 * Continuous image coordinates: pixel (row i, col j) covers [j, j+1) x [i, i+1).
 * ---------------------------------------------------------------------- */
/* Pointwise colour step: src, dst [B,H,W,3] uint8 (different buffers, 4-byte aligned), color [B,3] f32 = (grayscale
 * alpha, hue rotation in degrees, brightness add on V of HSV).  An image whose three values are 0 is copied. */
int cnuda_augment_color(const unsigned char* src, unsigned char* dst, const float* color, int B, int H, int W,
                        cnuda_stream_t stream);
/* One resampling per image.  src [B,Hmax,Wmax,3] uint8, sizes [B,2] int32 the valid (h, w) of each image (clamped to
 * the buffer), inverse [B,6] f32 the map from output to source coordinates (u = (a0 x + a1 y) + a2, v = (a3 x + a4 y)
 * + a5 at x = j + 0.5, y = i + 0.5), taps [B,10,3] f32 (offset x, offset y, weight) with ntaps [B] int32 (clamped to
 * 10) the motion-blur line in source space, noise [B] f32 the standard deviation of the additive gaussian noise (0 =
 * none), ids [B] int64 or NULL (= the position in the batch) the images' noise counters, seed the Philox4x32-10 key.
 * dst [B,Hin,Win,3] uint8, 4-byte aligned.  A pixel whose source point lies outside [0, w] x [0, h] is 0; otherwise
 * clamp(rint(sum_m weight_m * bilinear(u + ox_m - 0.5, v + oy_m - 0.5) + noise), 0, 255) with replicated edges. */
int cnuda_augment_warp(const unsigned char* src, unsigned char* dst, const int* sizes, const float* inverse,
                       const float* taps, const int* ntaps, const float* noise, const long long* ids,
                       unsigned long long seed, int B, int Hmax, int Wmax, int Hin, int Win, cnuda_stream_t stream);
/* Annotations through the forward matrices, in double: forward [B,6]; points [B,N,2] -> points_out (may alias);
 * boxes [B,M,4] (x1, y1, x2, y2) -> boxes_out, the bounding box of the four mapped corners.  N or M may be 0 (then
 * the two pointers may be NULL). */
int cnuda_augment_points(const double* forward, const double* points, double* points_out, int N,
                         const double* boxes, double* boxes_out, int M, int B, cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Detection previews (utils/visualize.py:23-49 behind utils/tensorboard.py:21-44 of the reference, restated as pixel
 * rules: DESIGN.md, "Detection previews on the device").  One launch paints n images of the batch twice, side by side:
 *   input [B,3,H,W] f32 the normalised batch, index [n] int32 which images to render (an index outside [0, B) renders
 *   over black), out [n,3,H,2W] uint8 with the prediction panel in columns [0, W) and the ground-truth panel in
 *   [W, 2W).  H, W <= 8192, n <= 65535.
 * Base pixel of both panels: v = (x * std_c + mean_c) * 255, each step one float32 operation, clamped to [0, 255] and
 * truncated toward zero.
 * prims [N, CNUDA_RENDER_RECORD] int32 (16-byte aligned), first [n+1] int32: rendered image i takes the records
 * [first[i], first[i+1]) (clamped to [0, N]), applied IN LIST ORDER.  A record is 16 words:
 *   0 kind (CNUDA_RENDER_RING / _FILL / _QUAD / _GLYPH; anything else is skipped), 1 panel (0 prediction, 1 ground truth;
 *   anything else is skipped), 2 colour r | g << 8 | b << 16, 3 alpha (the bits of a float32 in [0, 1]),
 *   4 thickness t (RING, QUAD; clamped to [0, 1024]) or glyph index g (GLYPH; outside [0, G) is skipped),
 *   5..12 geometry in panel-local pixels, x = column, y = row, each clamped to [-32768, 32767]:
 *           RING, FILL x1, y1, x2, y2;  QUAD x0, y0, x1, y1, x2, y2, x3, y3;  GLYPH x0, y0 (the cell's origin),
 *   13..15 reserved (0).
 * A pixel (x, y) of the record's own panel is covered iff
 *   RING   x1-t+1 <= x <= x2+t-1 and y1-t+1 <= y <= y2+t-1 and not (x1 < x < x2 and y1 < y < y2);
 *   FILL   x1 <= x <= x2 and y1 <= y <= y2;
 *   QUAD   4 d^2 <= t^2 for the distance d to one of the four segments of the closed outline, in exact integers: with
 *          e = Q - P, w = X - P, L = e.e, s = w.e:  s <= 0: 4 |w|^2 <= t^2;  s >= L: 4 |X - Q|^2 <= t^2;  else
 *          4 (w x e)^2 <= t^2 L (a zero-length edge is its end point);
 *   GLYPH  0 <= x - x0 < gw and 0 <= y - y0 < gh; its alpha is float(atlas[g, y - y0, x - x0]) / 255.0f, the record's
 *          alpha is ignored.  atlas [G, gh, gw] uint8 coverage (G may be 0 and atlas NULL; gh, gw <= 256).
 * and then, per channel, v = rint(v + alpha * (c - v)) in float32: one subtract, one multiply, one add, round half to
 * even; the pixel is a byte again after every record.  Nothing crosses the seam between the panels.
 * A gather without atomics: bit-stable.  CNUDA_RENDER_CHUNK records are tested and compacted per pass of a workgroup. */
#define CNUDA_RENDER_RECORD 16
#define CNUDA_RENDER_CHUNK 256
#define CNUDA_RENDER_RING 0
#define CNUDA_RENDER_FILL 1
#define CNUDA_RENDER_QUAD 2
#define CNUDA_RENDER_GLYPH 3
int cnuda_render_detections(const float* input, const int* index, const int* prims, const int* first,
                            const unsigned char* atlas, unsigned char* out, int B, int n, int H, int W, int N,
                            int G, int gh, int gw, float mean0, float mean1, float mean2,
                            float std0, float std1, float std2, cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Running statistics on the device (the driver's AverageMeter bookkeeping, train.py:162-166, without a read-back per
 * statistic and step).  values: a HOST array of S (1..32) device pointers to float32 scalars; they are passed to the
 * kernel by value, nothing is uploaded.  sum [S] f64, count [S] f64 and last [S] f32 are device arrays; meter i does
 *   sum[i] = sum[i] + (double)v_i * n;  count[i] = count[i] + n;  last[i] = v_i
 * with the product and the sum rounded separately (no fused multiply-add): the float64 sequence of
 * AverageMeter.update(float(v), n).  One launch of one 64-lane workgroup, no atomics.  Null pointers, S outside 1..32
 * and n < 0 (or NaN) return CNUDA_ERR_INVALID_ARGUMENT without a launch. */
int cnuda_meter_update(const float* const* values, int S, double n, double* sum, double* count, float* last,
                       cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Prediction over images (predict.py; csrc/predict.hip; DESIGN.md, "Prediction").  Deterministic: no floating-point
 * atomics, every result independent of scheduling.  Caller's stream.
 * ---------------------------------------------------------------------- */
/* y[p, i, j] = x[p, i, W-1-j] for `planes` planes of H x W float32 (an input batch [B,3,H,W]: planes = 3 B).  A copy:
 * bit-exact.  x and y must not overlap. */
int cnuda_mirror_input(const float* x, float* y, long long planes, int H, int W, cnuda_stream_t stream);
/* Mirror test-time augmentation: the RAW head maps of a 2B batch -- images 0..B-1 and their left-right mirrors
 * B..2B-1 -- to B merged maps (M = the mirror j -> W-1-j), float32, one rounding per output:
 *   hm_out[b]  = 0.5 (s(hm[b]) + M s(hm[B+b])), s = clamp(sigmoid, 1e-4, 1 - 1e-4) as cnuda_sigmoid_clamp_ computes it
 *                (hm_out is what decode_detection takes: no further sigmoid);      hm [2B,C,H,W] -> [B,C,H,W]
 *   wh_out[b]  = 0.5 (wh[b] + M wh[B+b]) for channels 0, 1; a third channel (the angle) is wh[b]'s; wh [2B,wh_ch,H,W]
 *   reg_out[b] = reg[b]                                     (reg, reg_out both NULL: the model has no offset head)
 *   kps_out[b]: x_j = 0.5 (kps[b][2j] - M kps[B+b][2 perm[j]]), y_j = 0.5 (kps[b][2j+1] + M kps[B+b][2 perm[j] + 1]);
 *               kps [2B,2J,H,W], perm [J] int32 on the device with values in [0, J) (NULL: the identity); J = 0: kps,
 *               kps_out and perm NULL. */
int cnuda_tta_merge(const float* hm, const float* wh, const float* reg, const float* kps, const int* perm,
                    float* hm_out, float* wh_out, float* reg_out, float* kps_out,
                    int B, int C, int wh_ch, int J, int H, int W, cnuda_stream_t stream);
/* Decoded detections to source-image pixels.  dets [B,K,6] (x1, y1, x2, y2, score, class) or, rotated, [B,K,7]
 * (cx, cy, w, h, angle in degrees, score, class) as cnuda_decode_detection leaves them, rows in descending score order;
 * the four geometry columns (and kps [B,K,J,2], NULL with J = 0) are first multiplied by `scale` in float32 (the
 * model's down_ratio; 1: already input pixels).  matrix [B,6] float64: input -> source pixels, row-major 2 x 3,
 * X = (m0 x + m1 y) + m2, Y = (m3 x + m4 y) + m5; sizes [B,2] int32 (h, w) of the sources.  All arithmetic in double,
 * stored as float32.  Outputs are arrays of out_rows >= out_first + K rows per image; row k of the call lands in row
 * out_first + k (several scales write one candidate table):
 *   axis-aligned: boxes [B,out_rows,4], the bounding box of the four mapped corners clipped to [0, w] x [0, h];
 *   rotated: boxes [B,out_rows,4,2], the vertices centre + (-w/2,-h/2), (w/2,-h/2), (w/2,h/2), (-w/2,h/2) times
 *     [[cos, sin], [-sin, cos]] (utils/box.py rotate_bboxes, not truncated), mapped, not clipped;
 *   scores [B,out_rows], classes [B,out_rows] int32, kps_out [B,out_rows,J,2] (mapped, not clipped);
 *   counts [B] int32: the rows of this call with score >= threshold (both float32; a prefix, given the order). */
int cnuda_project_detections(const float* dets, const float* kps, const double* matrix, const int* sizes,
                             float* boxes, float* scores, int* classes, float* kps_out, int* counts,
                             int B, int K, int J, int rotated, float scale, float threshold,
                             int out_rows, int out_first, cnuda_stream_t stream);
/* Gaussian soft-NMS over the candidates of several scales, per image.  boxes [B,N,4] (x1, y1, x2, y2), scores [B,N],
 * classes [B,N] int32 (outside [0, C): ignored), kps [B,N,J,2] or NULL (J = 0); ncand [B] int32 or NULL: image b
 * uses its first ncand[b] (clamped to [0, N]) candidates, all N with NULL.  N <= CNUDA_SOFT_NMS_MAX_CANDIDATES, else
 * an error (never truncated).  Stage 1, per (image, class), in double: area = (x2-x1)(y2-y1); iou = inter /
 * ((a_i + a_j) - inter), 0 without overlap or with a union <= 0; repeat: take the live candidate with the largest
 * current score (ties: the lower candidate index); stop when it is < 1e-3; else emit it with that score and multiply
 * every other live candidate's score by exp(-(iou iou) / 0.5).  Stage 2, per image: the emitted candidates ordered by
 * (score descending, class ascending, index ascending), the first max_detections kept: out_boxes [B,max_detections,4],
 * out_scores (float32 of the double), out_classes int32, out_kps [B,max_detections,J,2]; rows past the last kept one
 * are zero with class -1.  counts [B]: kept rows with float32 score >= threshold.
 * Workspace: cnuda_predict_workspace_bytes(B, N) (0 and an error text when N is over the limit). */
#define CNUDA_SOFT_NMS_MAX_CANDIDATES 2048
size_t cnuda_predict_workspace_bytes(int B, int N);
int cnuda_soft_nms_merge(const float* boxes, const float* scores, const int* classes, const float* kps,
                         const int* ncand, float* out_boxes, float* out_scores, int* out_classes, float* out_kps,
                         int* counts, int B, int N, int C, int J, int max_detections, float threshold,
                         void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* cnuda_soft_nms_merge on rotated boxes: boxes [B,N,4,2] and out_boxes [B,max_detections,4,2] are quadrilaterals (x, y)
 * as cnuda_project_detections writes them, and iou = cnuda_quad_iou_pairs' exact polygon IoU with the round's winner as
 * subject and the candidate as clipper.  Everything else -- the two stages, the (score, class, index) keys, the 1e-3
 * stop, the decay, ncand, kps, counts, the candidate limit, the workspace -- is cnuda_soft_nms_merge's (the same two
 * kernels on another box record; the 2048 quads of a class sit in 64 KiB of LDS beside the scores: 88 KiB static). */
int cnuda_soft_nms_merge_rotated(const float* boxes, const float* scores, const int* classes, const float* kps,
                                 const int* ncand, float* out_boxes, float* out_scores, int* out_classes,
                                 float* out_kps, int* counts, int B, int N, int C, int J, int max_detections,
                                 float threshold, void* workspace, size_t workspace_bytes, cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Rotated IoU (hip_runtime.ops.rotated_iou; csrc/polyiou.cuh, csrc/polyiou.hip; DESIGN.md, "Rotated IoU"): the exact
 * IoU of two convex quadrilaterals in float64.  a [B,N,4,2], b [B,M,4,2] float32 (x, y) vertices in either winding;
 * iou [B,N,M] double; area_a [B,N], area_b [B,M] double, each may be NULL.  Per pair, subject a, clipper b:
 *   1. a coordinate that is not finite: iou 0 (and that quad's area 0);
 *   2. a2 = sum_{i=0..3} (x_i y_{i+1} - x_{i+1} y_i), ascending i into one accumulator that starts at 0, indices mod 4;
 *      a2 < 0: the vertex order becomes 3, 2, 1, 0 and a2 is negated; area = a2 / 2; a2 of a or of b not > 0: iou 0;
 *   3. Sutherland-Hodgman over the edges k = 0..3 of b, a = b_k, e = b_{k+1} - a, d(p) = e.x (p.y - a.y) - e.y (p.x - a.x):
 *      for the vertices p_j of the current polygon with successor q, emit p when d(p) >= 0, then p + t (q - p) with
 *      t = d(p) / (d(p) - d(q)) when d(p) and d(q) have strictly opposite signs; an empty polygon ends the clipping;
 *   4. i2 = the sum of 2 over the result (0 below three vertices), clamped to [0, min(a2_a, a2_b)];
 *      u2 = a2_a + a2_b - i2; iou = i2 / u2 when u2 > 0, else 0.
 * Doubles, + - * / and comparisons only, no fused multiply-add: the bits of the same steps in any IEEE float64
 * arithmetic (tests/polyiou_oracle.py).  A convex subject never exceeds 8 vertices; a quad that is not convex or
 * crosses itself gives a finite value in [0, 1] that is otherwise unspecified (vertices past the eighth are dropped).
 * One launch, no workspace, no atomics.  B > 0; N or M may be 0.
 * ---------------------------------------------------------------------- */
int cnuda_quad_iou_pairs(const float* a, const float* b, double* iou, double* area_a, double* area_b,
                         int B, int N, int M, cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Mean teacher (uda/mean_teacher.py; csrc/teacher.hip; DESIGN.md, "Mean teacher").  No reference counterpart.  No
 * atomics: every result is independent of scheduling.  Caller's stream.
 * ---------------------------------------------------------------------- */
/* One launch over a DEVICE-resident table of `segments` entries of 32 bytes each,
 *   { void* dst; const void* src; long long count; int kind; unsigned block0; }
 * kind 0: count float32 elements, dst[i] = (dst[i] * decay) + (src[i] * one_minus_decay): two rounded products and one
 *         rounded sum, never contracted -- numpy's float32 `t * d + s * omd` bit for bit.  one_minus_decay must be
 *         float32(1) - decay, decay in [0, 1).  Both pointers 4-byte aligned; 16-byte accesses are taken only at
 *         elements where BOTH are 16-byte aligned (a scalar head and tail around them), scalar accesses otherwise.
 * kind 1: count bytes, dst[i] = src[i] (integer buffers such as num_batches_tracked); any alignment.
 * A segment owns the workgroups block0 .. block0 + ceil(count / 4096) - 1 (none when count == 0); block0 is the running
 * sum over the table and `blocks` its total.  dst and src ranges must not overlap.  The table's contents are the caller's
 * responsibility (hip_runtime.ops.EmaPlan); segments == 0 or blocks == 0 launch nothing. */
int cnuda_ema_update(const void* table, int segments, unsigned blocks, float decay, float one_minus_decay,
                     cnuda_stream_t stream);
/* A decoded detection table to the inputs of cnuda_encode_targets_modes, at output-map resolution.  dets [B,K,6]
 * (x1, y1, x2, y2, score, class) or, rotated, [B,K,7] (cx, cy, w, h, angle in degrees, score, class); thresholds [C]
 * float32.  A row survives iff its class is an integer in [0, C), score >= thresholds[class] (float32, equality keeps),
 * its geometry columns are all finite and both extents (x2 - x1 and y2 - y1 in double; w and h when rotated) are
 * >= min_size.  Survivors are compacted to the front in input order (stable); the other rows of every output are zero.
 *   classes [B,K] int32, counts [B] int32, kept: one float32 = float32(double(sum of counts) / B);
 *   geometry, axis-aligned: [B,K,4] float64 (x1, y1, x2, y2), with mirror != 0 (map_width - x2, y1, map_width - x1, y2);
 *   geometry, rotated: [B,K,4,2] float64, the vertices of cnuda_project_detections (centre + (-w/2,-h/2), (w/2,-h/2),
 *     (w/2,h/2), (-w/2,h/2) rotated by the angle, in double), with mirror != 0 every vertex's x -> map_width - x. */
int cnuda_pseudo_labels(const float* dets, const float* thresholds, double* geometry, int* classes, int* counts,
                        float* kept, int B, int K, int C, int rotated, int mirror, int map_width, float min_size,
                        cnuda_stream_t stream);
/* cnuda_pseudo_labels with the detections' decoded keypoints (uda.KeypointTeacher; DESIGN.md, "Keypoint teacher"):
 * kps [B,K,J,2] float32 (x, y) at map resolution, as cnuda_decode_keypoints leaves them; perm [J] int32 or null (the
 * identity): the joint that takes joint j's place in a mirrored image.  Row survival is cnuda_pseudo_labels' rule -- the
 * joints never decide it -- and geometry, classes, counts and kept are its results bit for bit.  In addition, for the
 * survivor in slot s that was input row k, output joint j takes input joint p = perm[j]:
 *   x' = mirror ? (double)map_width - (double)x : (double)x,  y' = (double)y          (the rule of the box edges)
 *   v = 2 iff x and y are finite, 0 <= x' < map_width and 0 <= y' < map_height; else v = 0
 *   keypoints [B,K,J,2] float64 = (x', y'), visibility [B,K,J] int32 = v; a joint that is not finite is (0, 0) with v = 0,
 *   and so is one whose perm entry lies outside [0, J) (nothing is read for it).
 * Rows behind the survivors are zero in every output.  joints: one float32 = float32(double(number of v = 2) / B), from
 * integer counts.  One launch, one wave per image, no atomics: the same bits on every run.  Any J > 0. */
int cnuda_pseudo_labels_kps(const float* dets, const float* kps, const float* thresholds, const int* perm,
                            double* geometry, int* classes, int* counts, float* kept, double* keypoints, int* visibility,
                            float* joints, int B, int K, int C, int J, int rotated, int mirror, int map_height,
                            int map_width, float min_size, cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Strong view (datasets/strong_view.py, uda.WeakStrongTeacher; csrc/strongview.hip; DESIGN.md, "Strong view").  No
 * reference counterpart.  Colour jitter, grayscale, gaussian blur and random erasing on a normalised batch
 * x [B,3,H,W] f32 (channel 0 = R), drawn on the host and applied from per-image DEVICE tables.  Every float32 step is
 * one IEEE operation in the written order, only + - * / min max: numpy's float32 arithmetic bit for bit.  Caller's stream.
 * With v_c = clamp(x_c * std_c + mean_c, 0, 1) and luma(v) = (0.299f v_R + 0.587f v_G) + 0.114f v_B:
 * ---------------------------------------------------------------------- */
/* pivot[b] = the mean luma of image b before any step: q = (unsigned)rintf(luma(v) * 65536.0f) per pixel, summed in
 * 64-bit integers (atomics on an integer: the same bits on every run), pivot = (float)((double)sum / (65536.0 H W)).
 * mean, std [3] and pivot [B] on the device; workspace: 16 B bytes on the device, 8-byte aligned, cleared here. */
int cnuda_strong_view_pivot(const float* x, const float* mean, const float* std, float* pivot, void* workspace,
                            int B, int H, int W, cnuda_stream_t stream);
/* y [B,3,H,W] f32, a buffer that does not overlap x (x is never written).  Tables, all on the device:
 *   photo [B,4] f32 (brightness fb, contrast fc, saturation fs, gray flag 0 / 1); taps [B,13] f32 with radius [B] int32
 *   (image b blurs with taps[b, 0 .. 2 radius[b]]; radius is clamped to 0..max_radius, max_radius <= 6 is the caller's
 *   statement of the largest one); rects [B,3,4] int32 (x0, y0, x1, y1) half-open, empty when x1 <= x0 or y1 <= y0;
 *   ids [B] int64; pivot [B] f32, read only for images with fc != 1 (cnuda_strong_view_pivot).
 * Per image, in this order; a factor that is exactly 1 skips its step:
 *   1 brightness  v_c = min(v_c fb, 1)                          2 contrast    v_c = clamp((v_c - pivot) fc + pivot, 0, 1)
 *   3 saturation  g = luma(v), v_c = clamp((v_c - g) fs + g, 0, 1)   4 gray   v_c = luma(v)
 *   5 blur        horizontal pass, its float32 result kept, then the vertical pass; each is acc = 0, then for k
 *                 ascending acc = acc + taps[k] v[at + k - radius] with neighbour indices clamped to the image;
 *                 radius 0 skips it
 *   6 out         y_c = (v_c - mean_c) / std_c
 * Inside a non-empty rectangle y_c = (u_c * 2 - 1) * 1.7320508f instead, u_c = ((float)(word_c >> 9) + 0.5f) / 2^23,
 * word_0..2 from the Philox4x32-10 block with key = seed and counter = (pixel index y W + x, ids[b]): the value of a
 * pixel depends on (seed, id, pixel) alone.  An image with fb = fc = fs = 1, no gray and radius 0 is neutral: outside
 * rectangles y has x's bits (the round trip through v is not exact and is not taken). */
int cnuda_strong_view(const float* x, float* y, const float* mean, const float* std, const float* photo,
                      const float* taps, const int* radius, int max_radius, const int* rects, const long long* ids,
                      unsigned long long seed, const float* pivot, int B, int H, int W, cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Geometric view (datasets/geometric_view.py, uda.GeometricTeacher; csrc/geomview.hip; DESIGN.md, "Geometric view").  No
 * reference counterpart.  A similarity transform of a normalised batch and of the teacher's pseudo-labels.  Coordinates
 * are those of datasets/augment.py: pixel (row i, column j) has its centre at (j + 0.5, i + 0.5); a matrix is the
 * row-major 2 x 3 part (m0 .. m5) of a 3 x 3 float64 matrix acting on columns (x, y, 1).  No atomics, caller's stream.
 * ---------------------------------------------------------------------- */
/* y [B,C,H,W] f32 = the bilinear resampling of x [B,C,H,W] f32 (contiguous, not overlapping; x is never written) under
 * inverse [B,6] float64 on the DEVICE: output pixel centres -> source positions.  Per output pixel (i, j) of image b:
 *   dx = (double)j + 0.5, dy = (double)i + 0.5                                   (doubles, one rounding per operation)
 *   u = ((m0 dx + m1 dy) + m2) - 0.5,   v = ((m3 dx + m4 dy) + m5) - 0.5
 *   x0 = floor(u), y0 = floor(v),   fx = (float)(u - x0), fy = (float)(v - y0)
 *   a, b, c, d = x[y0, x0], x[y0, x0 + 1], x[y0 + 1, x0], x[y0 + 1, x0 + 1]; a tap outside the image has the value `fill`
 *   per channel, in float32:  top = a + fx (b - a),  bot = c + fx (d - c),  y = top + fy (bot - top)
 * Every step is one IEEE operation, never contracted: numpy's arithmetic bit for bit (tests/geometric_view_oracle.py).
 * Weights of exactly 0 (a mirror, a half turn, a shift by whole pixels, a quarter turn of a square image) reproduce the
 * tap a for finite data (a = -0 comes out as +0).  An image whose six entries are exactly (1, 0, 0, 0, 1, 0) is copied
 * and keeps every bit.  One launch; H W + W + 1 < 2^31. */
int cnuda_warp_bilinear(const float* x, float* y, const double* inverse, float fill, int B, int C, int H, int W,
                        cnuda_stream_t stream);
/* The pseudo-labels of cnuda_pseudo_labels under the view: geometry_in [B,K,4] float64 (x1, y1, x2, y2) or, rotated,
 * [B,K,4,2] float64 corners; classes_in [B,K] int32; counts_in [B] int32 (clamped to 0..K); forward [B,6] float64 on
 * the DEVICE, the view's matrix at output-map resolution (map cells -> map cells).  The outputs have the inputs' layouts
 * and are other buffers; the inputs are not written.  Per row below its image's count, in float64, with
 * p' = ((m0 p.x + m1 p.y) + m2, (m3 p.x + m4 p.y) + m5):
 *   rotated       the four corners mapped point by point (the label, in their order); extent = |p1' - p0'|, |p2' - p1'|;
 *                 area and visible = area(quad clipped by [0, map_w] x [0, map_h]) / area(quad) by steps 1 to 4 of the
 *                 rotated IoU above with the quad as subject and the map's rectangle as clipper (csrc/polyiou.cuh:
 *                 the same routine), visible = i2 / a2;
 *   axis-aligned  the corners (x1, y1), (x2, y1), (x2, y2), (x1, y2) mapped; the label is their bounding box (min and max
 *                 per axis); extent = its width w and height h, area = w h,
 *                 visible = max(min(x2, map_w) - max(x1, 0), 0) max(min(y2, map_h) - max(y1, 0), 0) / area.
 * A row survives iff both extents >= min_size, its area is positive and finite (every mapped coordinate finite) and
 * visible >= min_visible.  An image whose six entries are exactly (1, 0, 0, 0, 1, 0) keeps every row as it is.
 * Survivors are compacted to the front in input order, unclipped; the other rows of every output are zero.
 *   counts_out [B] int32; kept = float32(double(sum counts_out) / B);
 *   dropped = float32(double(sum counts_in - sum counts_out) / B).
 * Two launches: one workgroup per image (a ballot and a prefix count place the survivors), then the two means. */
int cnuda_labels_transform(const double* geometry_in, const int* classes_in, const int* counts_in, const double* forward,
                           double* geometry_out, int* classes_out, int* counts_out, float* kept, float* dropped, int B,
                           int K, int rotated, int map_h, int map_w, double min_size, double min_visible,
                           cnuda_stream_t stream);
/* cnuda_labels_transform with the rows' joints (cnuda_pseudo_labels_kps' keypoints [B,K,J,2] float64 and visibility
 * [B,K,J] int32): the same survival rule, compaction, kept and dropped -- the joints never decide a row's survival, and a
 * dropped row's joints disappear with it.  Every joint of a surviving row, in float64:
 *   p' = ((m0 x + m1 y) + m2, (m3 x + m4 y) + m5)
 *   v' = 2 iff v == 2, p' is finite, 0 <= p'.x < map_w and 0 <= p'.y < map_h; else v' = 0;  a p' that is not finite is
 *   written as (0, 0).
 * An image whose six entries are exactly (1, 0, 0, 0, 1, 0) keeps its joints and v as they are.  Rows behind the
 * survivors are zero.  joints = float32(double(number of v' = 2 in surviving rows) / B).  The outputs are other buffers than
 * the inputs.  Two launches: one wave per image, then the three means from integer sums.  Any J > 0. */
int cnuda_labels_transform_kps(const double* geometry_in, const int* classes_in, const int* counts_in,
                               const double* keypoints_in, const int* visibility_in, const double* forward,
                               double* geometry_out, int* classes_out, int* counts_out, double* keypoints_out,
                               int* visibility_out, float* kept, float* dropped, float* joints, int B, int K, int J,
                               int rotated, int map_h, int map_w, double min_size, double min_visible,
                               cnuda_stream_t stream);

/* -------------------------------------------------------------------------
 * Dense teacher (uda.DenseTeacher; csrc/dense.hip; DESIGN.md, "Dense teacher").  No reference counterpart: Dense
 * Teacher (Zhou et al., ECCV 2022) on CenterNet's heads.  All maps are contiguous fp32; teacher_hm, hm [B,C,H,W] are
 * LOGITS, teacher_wh, wh [B,2,H,W].  With HW = H W, the score s[b,p] = max_c teacher_hm[b,c,p] (NaN if any channel is),
 *   k = max(1, floor(ratio HW)) in double, tau[b] = the k-th largest s[b,.], M[b,p] = (s[b,p] >= tau[b]) as floats:
 * every tie at tau is selected, -0 equals +0 (a zero tau is stored as +0), a NaN score orders below every number and is
 * never selected; with fewer than k numbers in an image tau[b] = -inf (every number is selected, possibly none).
 * count[b] = |M[b]| >= k.  Position p = (y, x) of the teacher is p' = (y, W-1-x) of the student with mirror != 0, else p.
 *   y = sigmoid(teacher_hm) on M else 0, q = sigmoid(hm[p']), bce = max(x,0) - x y + log1p(exp(-|x|)), N = sum count
 *   hm_loss = sum (y - q)^2 bce / max(N, 1);   u = sigmoid(s) on M else 0
 *   wh_loss = sum u (|wh[b,0,p'] - teacher_wh[b,0,p]| + |wh[b,1,p'] - teacher_wh[b,1,p]|) / (sum u + 1e-4)
 *   out5 = {hm_weight hm_loss + wh_weight wh_loss, hm_loss, wh_loss, N, sum u}
 * Integer counters and fp64 sums in a fixed order: the same bits every run.  No call synchronises or reads back.
 * 0 < ratio <= 1, C <= 1024 (the class limit of the library's per-image tables), HW < 2^31.
 * ---------------------------------------------------------------------- */
/* Bytes of device workspace cnuda_dense_select needs (the [B,HW] score keys); 0 for an invalid shape. */
size_t cnuda_dense_select_workspace_bytes(int B, long long HW);
/* tau [B] float32, count [B] int32.  Two launches: the channel-max score keys, then one workgroup per image selects. */
int cnuda_dense_select(const float* teacher_hm, double ratio, float* tau, int32_t* count, int B, int C, long long HW,
                       void* workspace, size_t workspace_bytes, cnuda_stream_t stream);
/* workspace: cnuda_loss_workspace_bytes().  Two launches (the reduction and its one-workgroup tail). */
int cnuda_dense_teacher_forward(const float* hm, const float* wh, const float* teacher_hm, const float* teacher_wh,
                                const float* tau, const int32_t* count, float* out5, int B, int C, int H, int W,
                                int mirror, float hm_weight, float wh_weight, void* workspace, size_t workspace_bytes,
                                cnuda_stream_t stream);
/* grad_hm [B,C,H,W] and grad_wh [B,2,H,W] are written whole (zeros included) by ONE launch; upstream: one device float;
 * out5: what the forward wrote.  d/dx = (q - y) ((q - y)^2 + 2 q (1 - q) bce) / max(N, 1);  d/dwh = u sign(.) /
 * (sum u + 1e-4), sign(0) = 0. */
int cnuda_dense_teacher_backward(const float* hm, const float* wh, const float* teacher_hm, const float* teacher_wh,
                                 const float* tau, const float* out5, const float* upstream, float* grad_hm,
                                 float* grad_wh, int B, int C, int H, int W, int mirror, float hm_weight,
                                 float wh_weight, cnuda_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CENTERNET_UDA_HIP_H */
