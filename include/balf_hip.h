/*
 * balf_hip.h -- C ABI of libbalf_hip.so: the MI355X (gfx950) implementation of BALF's
 * keypoint-detection hot path (detector forward -> score map -> window-max NMS -> top-K).
 *
 * The reference is pure Python and has no FFI of its own; these entry points
 * are what a binding for this path replaces, one per reference call site:
 *
 *   balf_pack_weights        <- MLP_MA_DECODER.load_state_dict, reached from
 *                               balf/model/get_model.py:65-67 (load_test_pretrained_model)
 *   balf_forward             <- MLP_MA_DECODER.forward, balf/model/mlp_ma_decoder.py:278-285
 *                               (+ DetectorHead.forward, balf/model/decoder.py:16-30)
 *   balf_window_nms          <- remove_borders + apply_nms, balf/utils/test_utils.py:34-54
 *   balf_nms_topk            <- crop + remove_borders + apply_nms + get_point_coordinates /
 *                               find_index_higher_scores + final sort,
 *                               balf/utils/train_utils.py:437-452, balf/utils/test_utils.py:50-95
 *
 * Conventions: plain pointers and sizes only.  Every device buffer (inputs, outputs, workspace)
 * is owned by the caller; the library never allocates or frees device memory, never calls
 * hipDeviceSynchronize, and enqueues all work on the hipStream_t passed as `stream`
 * (as void*; NULL = the null stream).  No entry point synchronises the stream or reads anything back: where the amount
 * of work depends on the data (the rounds of balf_greedy_nms, the candidate pairs of balf_repeatability) the kernels
 * decide on the device, and a result that did not fit is reported in the outputs.  Every function returns BALF_OK (0)
 * or a negative BALF_ERR_* code and never throws.  Shapes are validated on the host before any launch.
 */
#ifndef BALF_HIP_H
#define BALF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BALF_ABI_VERSION 1

#define BALF_OK 0
#define BALF_ERR_ARG (-1)        /* null pointer, non-positive size, unsupported parameter        */
#define BALF_ERR_SHAPE (-2)      /* H/W not a multiple of 64, crop outside the padded map, K > H*W */
#define BALF_ERR_WORKSPACE (-3)  /* workspace smaller than *_workspace_bytes() says               */
#define BALF_ERR_ARCH (-4)       /* current device is not gfx950                                  */
#define BALF_ERR_LAUNCH (-5)     /* HIP reported an error at launch                               */

/* limits */
#define BALF_MAX_NMS_SIZE 32     /* window-max NMS footprint side (reference default 15)          */
#define BALF_MAX_TOPK 16384      /* num_points per image (reference configs use 1000..10000)      */

/* precision of the Linear-layer contractions (everything else is always fp32) */
#define BALF_PREC_FP32 0         /* v_mfma_f32_16x16x4_f32, exact fp32 fma chains                  */
#define BALF_PREC_FP16 1         /* f16 MFMA with SPLIT operands: every operand is carried as hi = f16(v) and
                                    lo = f16(v - hi), a product is hi*hi' + lo*hi' + hi*lo' accumulated in fp32
                                    (v_mfma_f32_32x32x16_f16 in the persistent kernels of the early stages,
                                    v_mfma_f32_16x16x32_f16 elsewhere; conv0 of stage 1 as exact f32 MFMA): score
                                    map within ~6e-6 of the fp32 reference.  Operands must stay inside the f16
                                    range (|v| < 6.5e4): see MLP_MA_DECODER.validate_fp16 on the Python side     */

int balf_abi_version(void);
const char *balf_error_string(int code);
/* BALF_OK iff the current HIP device is a gfx950 part. */
int balf_device_check(void);
/* "release BALF_ABLATE_GELU=0 ..." for the library as shipped; "DIAGNOSTIC ..." with the switch values when it was built
 * with any of the timing-ablation / instrumentation switches of csrc/diag.h (wrong results: never to be deployed). */
const char *balf_build_flags(void);

/* ---- weights ------------------------------------------------------------------------------
 * The 166 floating-point state-dict tensors of MLP_MA_DECODER in state_dict() order
 * (num_batches_tracked, the one int64 entry, is skipped).  balf_state_tensor_name/numel let a
 * binding check its table against the library's.  balf_pack_weights runs on the HOST: it
 * reads `n_tensors` host pointers (contiguous fp32, nn.Linear layout [out,in]) and writes the
 * packed blob (MFMA-fragment-ordered weights, BatchNorm folded into the head) that the caller
 * then copies to the device and passes to balf_forward as `packed_dev`. */
int balf_num_state_tensors(void);
const char *balf_state_tensor_name(int i);
size_t balf_state_tensor_numel(int i);
size_t balf_packed_weights_bytes(int precision);
int balf_pack_weights(const float *const *tensors, int n_tensors, int precision,
                      void *packed_host, size_t packed_bytes);

/* ---- detector forward ---------------------------------------------------------------------
 * x_nchw_dev : [B,3,Hp,Wp] fp32, Hp and Wp multiples of 64 (callers pad: test_utils.py:23-32), Hp * Wp <= 2^25 pixels per
 *              image (e.g. 5792 x 5792; BALF_ERR_SHAPE beyond: the kernels use 32-bit byte offsets inside an image)
 * logits_dev : [B,65,Hp/8,Wp/8] fp32 (post-BatchNorm, pre-softmax), may be NULL to skip
 * prob_dev   : [B,Hp,Wp] fp32 score map (softmax over 65, dustbin dropped, pixel-shuffled)
 * workspace  : balf_forward_workspace_bytes(B,Hp,Wp) bytes, 256-byte aligned */
size_t balf_forward_workspace_bytes(int B, int Hp, int Wp);
/* Images per launch: the forward walks a batch in micro-batches of this many images (the workspace holds one micro-batch:
 * 16 images at 1088x1920, more at smaller sizes; B if the batch is smaller).  0: bad arguments. */
int balf_forward_micro_batch(int B, int Hp, int Wp);
int balf_forward(const void *packed_dev, int precision, const float *x_nchw_dev, int B, int Hp, int Wp,
                 float *logits_dev, float *prob_dev, void *workspace_dev, size_t workspace_bytes,
                 void *stream);

/* Same forward, fed with the raw uint8 image(s): gray [B,H,W] (channels = 1, replicated to the three input
 * channels) or RGB [B,H,W,3] (channels = 3).  The /255, make_shape_even and mod_padding_symmetric(64) of the
 * callers (demo/demo_match.py:22-29, balf/utils/test_utils.py:16-32) happen inside the first kernels; the
 * outputs have the PADDED size: Hp = H rounded up to even then to a multiple of 64 (same for W), the image at
 * rows (Hp-He)/2.., i.e. prob_dev [B,Hp,Wp], logits_dev [B,65,Hp/8,Wp/8], workspace for (B,Hp,Wp).  Results
 * are bit-identical to balf_forward on the host-prepared float input. */
int balf_forward_u8(const void *packed_dev, int precision, const unsigned char *image_dev, int channels, int B,
                    int H, int W, float *logits_dev, float *prob_dev, void *workspace_dev, size_t workspace_bytes,
                    void *stream);

/* The same two forwards with a STATUS WORD BLOCK: status_dev -> 4 ints, caller-owned, writable by the device (device memory, or
 * pinned host memory mapped into the device's address space so that the host can look at it without a copy), zeroed by the
 * caller.  The split-f16 path (BALF_PREC_FP16) carries every MFMA operand as two f16 halves: a value beyond +-65504
 * saturates the high half and beyond ~1.3e5 turns into inf / NaN without any trap (csrc/split16.h).  With a status block the
 * kernels report that, at no cost while nothing happens -- the library only ever STORES 1 into a word, it never clears one:
 *   status[BALF_STATUS_SCORE] = 1   a pixel's softmax denominator was not a positive finite number (head kernel): the score
 *                                   map of this call holds non-finite values or garbage;
 *   status[BALF_STATUS_RANGE] = 1   a stage output (the next stage's input, the head's input or conv2's output) reached
 *                                   |v| >= 65504: its high half saturated -- the low half alone (11 bits) carries the
 *                                   excess, precision drops from 2^-20 to ~3e-4 relative, and beyond ~1.3e5 it overflows too;
 *   status[BALF_STATUS_SE]    = 1   a squeeze-excite pre-activation was not finite (SE kernel);
 *   status[3]                       reserved (never written).
 * The words are valid once the stream has passed the call.  status_dev may be NULL (then these are balf_forward /
 * balf_forward_u8).  The exact-fp32 path (BALF_PREC_FP32) has no operand range to leave: it reports BALF_STATUS_SCORE and
 * BALF_STATUS_SE (its SE kernel is the same one).  BALF_STATUS_RANGE covers STAGE BOUNDARIES only (a stage's output, the
 * head's input, conv2's output); an overflow inside a stage (token mix, dense2 inputs) is seen only if it reaches a
 * boundary, the SE pre-activation or the softmax denominator; NaNs do not raise RANGE (the comparison is false for them).
 * Host mirror: MLP_MA_DECODER checks the block lazily and re-runs a flagged batch on the fp32 kernels. */
#define BALF_STATUS_SCORE 0
#define BALF_STATUS_RANGE 1
#define BALF_STATUS_SE 2
#define BALF_STATUS_WORDS 4
int balf_forward_status(const void *packed_dev, int precision, const float *x_nchw_dev, int B, int Hp, int Wp,
                        float *logits_dev, float *prob_dev, void *workspace_dev, size_t workspace_bytes,
                        int *status_dev, void *stream);
int balf_forward_u8_status(const void *packed_dev, int precision, const unsigned char *image_dev, int channels, int B,
                           int H, int W, float *logits_dev, float *prob_dev, void *workspace_dev, size_t workspace_bytes,
                           int *status_dev, void *stream);

/* Validation aid (not part of the data path): the activation that crosses stage boundary `stage` of the forward that last
 * ran on `workspace_dev` with the same (precision, B, Hp, Wp), as plain fp32 NHWC in out_dev:
 *   stage 1..3  Down.forward's return value of down1..down3 (mlp_ma_decoder.py:223-244: after MaxPool2d), i.e. the next
 *               stage's input: [B, Hp/2^s, Wp/2^s, C_s], C = 32/64/128 (the split-f16 path keeps these as hi+lo f16
 *               fragments in the workspace; the view adds the halves);
 *   stage 4     x2 = t * s + x1 + x0 of down4 BEFORE its conv2 (:239-241; conv2 runs inside the head kernel and its output
 *               never exists in memory): [B, Hp/8, Wp/8, 256] -- apply down4.conv2 to compare with the reference's down4.
 * Only the last micro-batch of a forward is resident in the workspace: B must not exceed it (BALF_ERR_ARG otherwise;
 * balf_forward_micro_batch: 16 images at 1088x1920, more at smaller sizes).  balf_forward_stage_view_numel = elements of out_dev (0: bad arguments). */
size_t balf_forward_stage_view_numel(int B, int Hp, int Wp, int stage);
int balf_forward_stage_view(int precision, const void *workspace_dev, size_t workspace_bytes, int B, int Hp, int Wp, int stage,
                            float *out_dev, void *stream);

/* ---- window-max NMS, dense form (apply_nms) ------------------------------------------------
 * score_dev [B,H,W] fp32 -> out_dev [B,H,W] fp32 = rb * (rb == max over the clipped
 * nms_size x nms_size window), rb = score with a `border`-pixel frame zeroed. */
int balf_window_nms(const float *score_dev, int B, int H, int W, int border, int nms_size,
                    float *out_dev, void *stream);

/* ---- crop + border + NMS + exact top-K ------------------------------------------------------
 * prob_dev [B,Hp,Wp]; the score map of image b is prob[b, crop_y:crop_y+H, crop_x:crop_x+W].
 * Outputs per image: idx_dev[b,0:count] flat indices y*W+x of the first K pixels in raster
 * order whose NMS score >= the K-th largest NMS score (reference fallback when that is <= 0),
 * emitted sorted by (score descending, index ascending); score_dev their scores;
 * entries past count are idx -1 / score 0.  K <= H*W (the reference raises IndexError
 * otherwise) and K <= BALF_MAX_TOPK.  Scores are probabilities (>= +0): with negative scores in the map the points
 * with a positive score are still selected exactly as the reference selects them, but the reference's <= 0 fallback
 * then returns -0.0 and negative window maxima (its NMS map is x * (x == max)), which this entry point does not
 * reproduce (it returns the first K raster pixels with score +0). */
size_t balf_nms_topk_workspace_bytes(int B, int H, int W, int K);
int balf_nms_topk(const float *prob_dev, int B, int Hp, int Wp, int crop_y, int crop_x, int H, int W,
                  int border, int nms_size, int K, int32_t *idx_dev, float *score_dev,
                  int32_t *count_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* The same selection with a caller-given threshold instead of the K-th largest score: `threshold != -1` of
 * find_index_higher_scores (/root/reference/balf/utils/test_utils.py:74-95): the first K pixels in raster order
 * with NMS score >= threshold (all of them if fewer reach it; count may be 0).  threshold must be > 0 and finite:
 * with a threshold <= 0 every pixel qualifies and the answer is the first K raster indices -- no device work, the
 * host mirror (balf_amd/utils/test_utils.py) returns those directly.  Same workspace as balf_nms_topk. */
int balf_nms_threshold(const float *prob_dev, int B, int Hp, int Wp, int crop_y, int crop_x, int H, int W,
                       int border, int nms_size, float threshold, int K, int32_t *idx_dev, float *score_dev,
                       int32_t *count_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- multi-scale extraction over an image pyramid (balf_amd/multiscale.py states the protocol) --------------------------
 * The Key.Net-style protocol that balf/configs/config_hpatches.py:50-80 configures (scale_factor_levels r, pyramid_levels P,
 * upsampled_levels U, num_points N): levels of scale r^(i-U), each run through balf_forward, a share of N points per level
 * chosen on the device, the level lists merged into one list in original-image coordinates with a scale column.
 *
 * balf_pyramid_level: one level into dst_dev [B,3,Hp,Wp] fp32, the zero-padded NCHW batch balf_forward takes (Hp, Wp, and
 * the image offset as in balf_forward_u8: H_out, W_out rounded up to even, then to a multiple of 64, centred); every
 * padded pixel is written (0 outside the image).  The source is
 *   BALF_PYR_SRC_U8     uint8 [B,H_in,W_in,channels], channels 1 (gray: replicated to the three planes) or 3; value / 255
 *   BALF_PYR_SRC_F32    fp32 [B,H_in,W_in,3]
 *   BALF_PYR_SRC_LEVEL  a level an earlier call wrote: fp32 [B,3,Hp_in,Wp_in] padded from H_in x W_in; channels = 1 reads
 *                       plane 0 only (a gray level's planes are equal)
 * sigma > 0: Gaussian blur first, taps exp(-k^2/2 sigma^2) for |k| <= R = int(4 sigma + 0.5) <= BALF_PYR_MAX_RADIUS,
 * normalised, half-sample symmetric border (scipy.ndimage mode='reflect'), separable; sigma <= 0: no blur.  Then bilinear
 * resampling to H_out x W_out with half-pixel centres: src = (o + 0.5) * in/out - 0.5 clamped below at 0, the upper
 * neighbour clamped to in - 1 (F.interpolate(mode='bilinear', align_corners=False)).  H_out = H_in, W_out = W_in without
 * blur is a copy: the level is then bit-identical to what balf_forward_u8 / pad_batch prepare.  fp32 arithmetic, the
 * sampling positions in float64: for sources in [0, 1] every pixel is within (4 R + 12) * 2^-24 of the float64 result.
 * Reduction limit: a 64-pixel output row's source footprint and blur halo are staged in LDS, two planes of
 * (3 + 2R) x (ceil(63 W_in / W_out) + 3 + 2R) floats in 64 KB at the least.  BALF_ERR_ARG beyond it: W_in / W_out above
 * ~43.28 without blur (ceil(63 W_in / W_out) <= 2727), ~18.46 at R = 2 (<= 1163), ~6.54 at R = 8 (<= 412); H_in / H_out is
 * not limited (the tile height shrinks from 8 rows to 1).  sigma >= 64, NaN or R > BALF_PYR_MAX_RADIUS: BALF_ERR_ARG. */
#define BALF_PYR_SRC_U8 0
#define BALF_PYR_SRC_F32 1
#define BALF_PYR_SRC_LEVEL 2
#define BALF_PYR_MAX_RADIUS 8
#define BALF_MAX_PYRAMID_LEVELS 32
int balf_pyramid_level(const void *src_dev, int src_kind, int channels, int B, int H_in, int W_in, double sigma, int H_out,
                       int W_out, float *dst_dev, void *stream);

/* balf_nms_topk with the K of each image decided ON THE DEVICE from a point budget:
 * K_b = min(max(cum_budget - taken_dev[b], 0), K_max, H*W) (never longer than a row, whatever taken_dev holds), then
 * taken_dev[b] += count_b.  Called once per level with cum_budget = the budget of the levels so far, a
 * level that finds fewer points than its share passes the rest down -- nothing is read back.  taken_dev [B] int32, zeroed by
 * the caller before the first level.  Rows are K_max long (idx_dev / score_dev [B,K_max], -1 / 0 past count_dev[b]);
 * 0 <= cum_budget <= K_max <= BALF_MAX_TOPK; K_max may exceed H*W.  Selection as balf_nms_topk, its <= 0 fallback included
 * (the first K_b raster pixels); K_b = 0 gives count 0.  Workspace: balf_nms_topk_workspace_bytes(B, H, W, 1). */
int balf_nms_topk_budget(const float *prob_dev, int B, int Hp, int Wp, int crop_y, int crop_x, int H, int W, int border,
                         int nms_size, int cum_budget, int K_max, int32_t *taken_dev, int32_t *idx_dev, float *score_dev,
                         int32_t *count_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* The L level lists -> one list per image in original-image coordinates.  idx_dev / score_dev [L,B,K_max] and count_dev
 * [L,B] as balf_nms_topk_budget writes them (flat index y * w + x in level l, w = level_w_host[l]).  Every entry is ordered
 * by (score descending, level ascending, flat index ascending); row r < count_out_dev[b] = min(total, N) of pts_dev
 * [B,N,4] float64 is the r-th entry's point (x, y, 1.0, score) mapped through h_host[9 l .. 9 l + 8] (row-major, HOST
 * memory) with the arithmetic of balf_apply_homography: (x', y', radius, score), or (y', x', radius, score) with order_yx.
 * Rows past the count are 0.  The entries of an image must fit min(L * K_max, BALF_MAX_TOPK) (budgeted lists sum to at most
 * N): an image whose lists hold more gets count -1 and zero rows.  L <= BALF_MAX_PYRAMID_LEVELS, N <= BALF_MAX_TOPK. */
int balf_multiscale_merge(const int32_t *idx_dev, const float *score_dev, const int32_t *count_dev, int L, int B, int K_max,
                          const int32_t *level_w_host, const double *h_host, int N, int order_yx, double *pts_dev,
                          int32_t *count_out_dev, void *stream);

/* ---- greedy "SuperPoint" NMS of the demo path --------------------------------------
 * Replaces get_points_direct_from_score_map + nms_fast (+ soft_argmax_points), balf/utils/test_utils.py:97-215,
 * as called by demo/demo_match.py:45-57.  The score map of image b is prob[b, crop_y:+H, crop_x:+W] with a
 * `border` frame zeroed; candidates = pixels >= conf_thresh (> 0); a candidate is kept iff no higher-scoring kept
 * candidate lies within Chebyshev distance dist_thresh (<= 16).  Output rows sorted by score descending (flat
 * index ascending among equal scores): idx_dev[B,K] (-1 padded), score_dev[B,K], count_dev[B] = rows returned
 * (<= K), total_dev[B] = points kept before truncation (may be NULL).  subpixel_patch > 0 additionally writes
 * xy_dev[B,K,2] = (x, y) refined by the patch soft-argmax.  The number of suppression rounds depends on the data
 * (4-8 on score maps, ~W / dist_thresh on a monotone ramp): a fixed number of rounds is enqueued, each returning at
 * once when nothing is alive, and a per-image kernel finishes whatever is left -- exact for every input, stream-ordered. */
size_t balf_greedy_nms_workspace_bytes(int B, int H, int W, int K);
int balf_greedy_nms(const float *prob_dev, int B, int Hp, int Wp, int crop_y, int crop_x, int H, int W, int border,
                    float conf_thresh, int dist_thresh, int K, int subpixel_patch, int32_t *idx_dev,
                    float *score_dev, float *xy_dev, int32_t *count_dev, int32_t *total_dev, void *workspace_dev,
                    size_t workspace_bytes, void *stream);

/* ---- NMS score maps: box_nms and apply_nms_fast of the evaluation configs, batched ---------------------
 * prob_dev [B,H,W] fp32 -> out_dev [B,H,W]: EVERY element is written, a survivor gets its score and every other element
 * +0.0f (the caller clears nothing); count_dev [B] = survivors per image after keep_top_k (may be NULL).
 *   BALF_NMS_MAP_GREEDY  apply_nms_fast(score_map, dist_thresh, conf_thresh) = get_nms_score_map_from_score_map(heatmap,
 *                        conf_thresh, nms_size = dist_thresh), benchmark_test/repeatability_tools.py:25-100: the kept list of
 *                        balf_greedy_nms on the candidates >= conf_thresh, 1 <= dist_thresh <= 16; footprint / radius ignored.
 *   BALF_NMS_MAP_BOX     box_nms(prob, size, iou, min_prob = conf_thresh, keep_top_k), :227-255: candidates >= conf_thresh,
 *                        visited in descending score order; one is kept iff no kept candidate lies at an offset (dr, dc) of
 *                        the FOOTPRINT = the offsets at which two size x size boxes have IoU > iou.  footprint (HOST memory,
 *                        copied into the kernels' argument block: nothing is uploaded) holds 2 * radius + 1 row words, bit
 *                        dc + radius of word dr + radius; 0 <= radius <= BALF_NMS_MAP_MAX_RADIUS; it must hold the centre, be
 *                        symmetric under (dr, dc) -> (-dr, -dc) and set no bit beyond 2 * radius.  dist_thresh ignored.
 * Equal scores, in both protocols and at the keep_top_k cut: the lower raster index first (the reference's order there is
 * whatever an unstable sort gives).  keep_top_k <= 0: all survivors.  conf_thresh > 0.  Stream-ordered, nothing synchronised
 * or read back, capturable; the number of rounds depends on the data and is finished by a per-image kernel as in
 * balf_greedy_nms.  BALF_ERR_ARG: an unknown protocol, B outside 1..65535, H or W < 1, conf_thresh <= 0 or NaN, dist_thresh
 * / radius / footprint outside the above, a NULL prob_dev, out_dev or workspace_dev; BALF_ERR_SHAPE: H * W >= 2^31;
 * BALF_ERR_WORKSPACE: fewer bytes than balf_nms_score_map_sizes gives (its output is written only with BALF_OK).  Every
 * refusal comes before any launch: the outputs are untouched. */
#define BALF_NMS_MAP_GREEDY 0
#define BALF_NMS_MAP_BOX 1
#define BALF_NMS_MAP_MAX_RADIUS 16
int balf_nms_score_map_sizes(int B, int H, int W, int protocol, size_t *workspace_bytes);
int balf_nms_score_map(const float *prob_dev, int B, int H, int W, int protocol, float conf_thresh, int dist_thresh,
                       const uint64_t *footprint, int radius, int keep_top_k, float *out_dev, int32_t *count_dev,
                       void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- HardNet patch descriptor of the demo path ----------------------------------------
 * Replaces HardNet.load_state_dict / HardNet.forward, third_party/hardnet/hardnet_pytorch.py:31-72, as called by
 * demo/demo_match.py:72-93,131-134.  The 21 floating-point state tensors in state_dict() order are, per
 * convolution i in features.{0,3,6,9,12,15,19}: weight [Cout,Cin,k,k], then the following BatchNorm's running_mean
 * and running_var (num_batches_tracked is skipped).  balf_hardnet_pack_weights runs on the HOST (BatchNorm folded,
 * split-f16 MFMA fragment order); the caller copies the blob to the device.
 * balf_hardnet_forward: patches_dev [N,32,32] fp32 (the [N,1,32,32] tensor HardNet.forward takes) ->
 * desc_dev [N,128] fp32, L2-normalised.  Contractions run on v_mfma_f32_16x16x32_f16 with split (hi+lo) operands,
 * fp32 accumulation: descriptors agree with the fp32 reference to ~1e-5. */
int balf_hardnet_num_state_tensors(void);
const char *balf_hardnet_state_tensor_name(int i);
size_t balf_hardnet_state_tensor_numel(int i);
size_t balf_hardnet_packed_weights_bytes(void);
int balf_hardnet_pack_weights(const float *const *tensors, int n_tensors, void *packed_host, size_t packed_bytes);
size_t balf_hardnet_workspace_bytes(int n_patches);
int balf_hardnet_forward(const void *packed_dev, const float *patches_dev, int n_patches, float *desc_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream);
/* Masked form for fixed-size keypoint slots: the patches are n_patches / group images x `group` slots, and only the
 * first count_dev[image] slots of each image are computed (the others cost nothing and get zero descriptors).
 * count_dev == NULL: as balf_hardnet_forward. */
int balf_hardnet_forward_masked(const void *packed_dev, const float *patches_dev, int n_patches, int group,
                                const int32_t *count_dev, float *desc_dev, void *workspace_dev, size_t workspace_bytes,
                                void *stream);
/* Same with a choice of operand precision: BALF_HARDNET_SPLIT_F16 (default everywhere else: hi+lo operands, three
 * products, descriptors within ~1e-6 of fp32) or BALF_HARDNET_PLAIN_F16 (one f16 product, activations stored as one
 * plane: about twice as fast, descriptors within ~5e-4 -- the accuracy class of the TF32 convolutions PyTorch uses
 * by default for this network on an NVIDIA GPU). */
#define BALF_HARDNET_SPLIT_F16 0
#define BALF_HARDNET_PLAIN_F16 1
int balf_hardnet_forward_ex(const void *packed_dev, const float *patches_dev, int n_patches, int group,
                            const int32_t *count_dev, int precision, float *desc_dev, void *workspace_dev,
                            size_t workspace_bytes, void *stream);

/* ---- patch extraction and descriptor matching of the demo path -------------------------
 * balf_extract_patches replaces kornia.feature.laf_from_center_scale_ori + extract_patches_from_pyramid(PS=32) as
 * called by demo/demo_match.py:62-70: gray_dev uint8 [H,W]; xy_dev [N,2] keypoint (x, y) in pixels; `scale` = the
 * LAF scale (args.s_mult) shared by all keypoints; patches_dev [N,32,32] fp32 in [0,1].
 * balf_match_smnn replaces kornia.feature.match_smnn(desc1, desc2, th) (demo_match.py:104-110): descriptors
 * [n,128] fp32; outputs idx_dev [min(n1,n2),2] (index in desc1, index in desc2; -1 padded, sorted by the first),
 * dist_dev [min(n1,n2)] (max of the two nearest/second-nearest distance ratios), count_dev [1].
 * Squared distances are formed in fp32 as |a|^2 + |b|^2 - 2 a.b (fp32 MFMA operands), within
 * 16 * 2^-24 * (|a| + |b|)^2 of the exact value; among exactly equal distances the lowest index is the
 * nearest neighbour.  Non-finite rows: a distance that comes out NaN (a row with a NaN, or with an Inf whose products
 * cancel) is never a nearest nor a second-nearest neighbour, as in torch.topk, where NaN sorts last -- such a row
 * matches nothing and the matches among the other rows are those of the call without it.  An all-zero row is an
 * ordinary descriptor.
 * kornia is a third-party dependency that is absent offline: both follow its published algorithm and are checked
 * against this repo's restatement only (parity unpinned). */
size_t balf_extract_patches_workspace_bytes(int H, int W, float scale);
int balf_extract_patches(const unsigned char *gray_dev, int H, int W, const float *xy_dev, int n_points, float scale,
                         float *patches_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* Batched form: gray_dev [B,H,W], xy_dev [B,K,2], count_dev [B] = keypoints actually present per image (NULL: all
 * K; slots past the count get zero patches), patches_dev [B,K,32,32].  One pyramid per image, one launch for all. */
size_t balf_extract_patches_batch_workspace_bytes(int B, int H, int W, float scale);
int balf_extract_patches_batch(const unsigned char *gray_dev, int B, int H, int W, const float *xy_dev,
                               const int32_t *count_dev, int K, float scale, float *patches_dev, void *workspace_dev,
                               size_t workspace_bytes, void *stream);
/* uint8 RGB (interleaved, n_pixels x 3) -> uint8 gray exactly as PIL's Image.convert('L') (demo_match.py:13-19). */
int balf_rgb_to_gray(const unsigned char *rgb_dev, long n_pixels, unsigned char *gray_dev, void *stream);
size_t balf_match_smnn_workspace_bytes(int n1, int n2);
/* Batched form: `pairs` independent problems, desc1_dev [pairs,k1,128] / desc2_dev [pairs,k2,128] with n1_dev / n2_dev
 * [pairs] valid rows each; idx_dev [pairs,min(k1,k2),2], dist_dev [pairs,min(k1,k2)], count_dev [pairs]. */
size_t balf_match_smnn_batch_workspace_bytes(int pairs, int k1, int k2);
int balf_match_smnn_batch(const float *desc1_dev, int k1, const int32_t *n1_dev, const float *desc2_dev, int k2,
                          const int32_t *n2_dev, int pairs, float th, int32_t *idx_dev, float *dist_dev,
                          int32_t *count_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int balf_match_smnn(const float *desc1_dev, int n1, const float *desc2_dev, int n2, float th, int32_t *idx_dev,
                    float *dist_dev, int32_t *count_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- repeatability evaluation ---------------------------------------------------------
 * balf_repeatability replaces compute_repeatability, balf/benchmark_test/repeatability_tools.py:379-490 (callers:
 * balf/utils/train_utils.py:189,257, balf/datasets/dataset_utils.py:332).  src_dev [ns,3] / dst_dev [nd,3] float64
 * rows (x, y, radius).  Outputs: counts_dev[3] = {num_points_single_scale, num_points_multi_scale,
 * possible_matches}; errors_dev[2] = the two sums of (1 - overlap) over the assigned pairs, in assignment order;
 * corr_s_dev / corr_m_dev [min(ns,nd),2] = (dst index, src index) per assigned pair in assignment order, -1 padded.
 * Among exactly equal overlaps the pair with the lower flat index ns-major wins (the reference's order there is
 * NumPy's unstable argsort).  max_edges bounds the number of pairs whose overlap reaches 1 - overlap_err, per scale;
 * that number is known on the device only: when a scale's list does not fit, its entry of counts_dev is -1 and its
 * correspondences are all -1 (the host mirror raises when it reads that) -- nothing waits for the device.
 * ns, nd <= 65536.
 * balf_apply_homography replaces apply_homography_to_points, balf/benchmark_test/geometry_tools.py:43-86:
 * points_dev [n,4] float64 rows (x, y, radius, score), h_dev[9] row-major -> out_dev [n,4]. */
size_t balf_repeatability_workspace_bytes(int ns, int nd, int max_edges);
int balf_repeatability(const double *src_dev, int ns, const double *dst_dev, int nd, double overlap_err, double eps,
                       double dist_match_thresh, double radius_size, int max_edges, int32_t *counts_dev,
                       double *errors_dev, int32_t *corr_s_dev, int32_t *corr_m_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);
int balf_apply_homography(const double *points_dev, int n, const double *h_dev, double *out_dev, void *stream);

/* create_common_region_masks, balf/benchmark_test/geometry_tools.py:7-26 (callers: the HPatches evaluation, and the
 * masks handed to compute_repeatability_with_maximum_filter, balf/utils/train_utils.py:170-196): the region of each
 * image covered by the other under the homography h_dst_2_src (HOST pointer, 9 doubles row-major).  mask_src_dev
 * [h_src, w_src] and mask_dst_dev [h_dst, w_dst] float64 in {0, 1}: cv2.warpPerspective of an all-ones image with a
 * zeroed `border` frame (bilinear, zero outside, source coordinates rounded to 1/32 pixel), >= 0.75, frame zeroed
 * again.  cv2 is absent from the build container: parity with it is unpinned. */
int balf_common_region_masks(const double *h_dst_2_src_host, int h_src, int w_src, int h_dst, int w_dst, int border,
                             double *mask_src_dev, double *mask_dst_dev, void *stream);

/* ---- batched HSequences evaluation (check_val_hsequences_repeatability, balf/utils/train_utils.py:308-413) ---------------
 * P independent image pairs, stream-ordered, nothing read back: every per-pair count is read on the device.
 *
 * balf_common_points_batch: what train_utils.py:350-369 does after detection, per pair p.  src_dev [P,ns_max,4] /
 * dst_dev [P,nd_max,4] float64 rows (x, y, radius, score), the first ns_dev[p] / nd_dev[p] of them used (clamped to
 * [0, n_max]); h_dst_2_src_dev [P,9] row-major, shapes_dev [P,4] int32 = (h_src, w_src, h_dst, w_dst).  A source row is kept
 * iff mask_src[round(y) - 1, round(x) - 1] != 0 (check_common_points: round half to even, a negative index wraps like
 * NumPy's, an index NumPy would reject drops the row), a destination row likewise against mask_dst, where the masks are
 * those balf_common_region_masks computes for the pair with border 15, evaluated at the point only (the two inverse maps are
 * computed on the device in the same operations).  Kept rows keep their order: src_out_dev [P,ns_max,4] the kept source rows,
 * dst_out_dev [P,nd_max,4] the kept destination rows warped as balf_apply_homography does (score carried); rows past the kept
 * count are 0.  kept_dev [P,2] = kept counts (source, destination); valid_dev[P] = both > 0.  A singular h_dst_2_src (the
 * closed-form determinant is exactly 0) and a pair whose shapes_dev row has an entry <= 0 keep nothing: kept (0, 0), valid 0,
 * every output row of the pair 0 (and every index -1); the other pairs of the batch are not affected.  Images smaller than
 * 31 x 31 have empty masks (the 15-pixel frame); a coordinate that is NaN, infinite or rounds outside [-n, n) drops its row.
 * No workspace.
 *
 * balf_repeatability_batch: balf_repeatability for each pair, bit-identical to it.  Rows of src_dev / dst_dev start with
 * (x, y, radius), src_stride / dst_stride doubles apart (>= 3); pair p's rows start at row p * ns_max / p * nd_max, its counts
 * are ns_dev[p * count_stride] / nd_dev[p * count_stride] (clamped to [0, n_max]).  max_edges bounds the candidate pairs of
 * each scale summed over ALL pairs: pair p's candidates take the slice after those of pairs < p, and a pair whose slice does
 * not end within max_edges reports found = -1 (and NaN rep / err) for that scale, its candidate count still written.
 * Outputs: rep_dev [P,4] float64 = (rep_single_scale, rep_multi_scale, error_overlap_single_scale,
 * error_overlap_multi_scale) with compute_repeatability's formulas (rep = found / total * 100, NaN for total 0; err = 0 for
 * found 0, else the error sum / (found + DBL_EPSILON)); counts_dev [P,6] int32 = (num_points_single_scale,
 * num_points_multi_scale, possible_matches, total_num_points = min(ns, nd), candidates single scale, candidates multi scale).
 * ns_max, nd_max <= 65536 (BALF_ERR_ARG), ns_max * nd_max < 2^31 (BALF_ERR_SHAPE), 1 <= P <= 65535. */
int balf_common_points_batch(const double *src_dev, const int32_t *ns_dev, int ns_max, const double *dst_dev,
                             const int32_t *nd_dev, int nd_max, int P, const double *h_dst_2_src_dev, const int32_t *shapes_dev,
                             double *src_out_dev, double *dst_out_dev, int32_t *kept_dev, int32_t *valid_dev, void *stream);
size_t balf_repeatability_batch_workspace_bytes(int P, int ns_max, int nd_max, int max_edges);
int balf_repeatability_batch(const double *src_dev, const int32_t *ns_dev, int ns_max, int src_stride, const double *dst_dev,
                             const int32_t *nd_dev, int nd_max, int dst_stride, int count_stride, int P, double overlap_err,
                             double eps, double dist_match_thresh, double radius_size, int max_edges, double *rep_dev,
                             int32_t *counts_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- matching score of the HSequences evaluation (the record fields mma, mma_corr, num_matches, num_mutual_corresp, avg_mma
 * of balf/benchmark_test/test_utils.py:create_results; the reference ships no code that fills them: DESIGN.md 7h defines them) --
 * balf_common_points_index_batch: balf_common_points_batch -- same arguments, same semantics, the same bits in the four
 * shared outputs -- plus src_index_dev [P,ns_max] / dst_index_dev [P,nd_max] int32: the original row of each kept row, in kept
 * order (strictly increasing), -1 past the kept count.  A per-image descriptor table is gathered through them.
 *
 * balf_match_accuracy_batch: the matches of P pairs verified against the homography.  src_dev [P,ns_max,4] / dst_dev
 * [P,nd_max,4] float64 are the kept lists (source rows; destination rows warped into the source image), kept_dev [P,2] their
 * lengths, match_idx_dev [P,cap,2] int32 the matches (row in src, row in dst) of which the first match_count_dev[p] are used
 * (counts clamped to [0, cap] / [0, n_max]); this is what balf_match_smnn_batch writes.  thresholds_host: T pixel thresholds
 * on the HOST, 1 <= T <= 16, >= 0 and strictly ascending; they are passed to the kernel as arguments (no upload).  Outputs:
 * err_dev [P,cap] float64 = sqrt(dx*dx + dy*dy) between the two matched rows, each operation rounded once (no FMA); NaN for a
 * slot past the count and for a match with an index outside [0, kept).  correct_dev [P,T] int32 = the matches with
 * err <= thresholds[k] (a NaN counts for none).  Every slot of both outputs is written.  1 <= cap <= 65536, the other limits
 * as above.  No workspace. */
int balf_common_points_index_batch(const double *src_dev, const int32_t *ns_dev, int ns_max, const double *dst_dev,
                                   const int32_t *nd_dev, int nd_max, int P, const double *h_dst_2_src_dev,
                                   const int32_t *shapes_dev, double *src_out_dev, double *dst_out_dev, int32_t *kept_dev,
                                   int32_t *valid_dev, int32_t *src_index_dev, int32_t *dst_index_dev, void *stream);
int balf_match_accuracy_batch(const double *src_dev, int ns_max, const double *dst_dev, int nd_max, const int32_t *kept_dev,
                              const int32_t *match_idx_dev, const int32_t *match_count_dev, int cap, int P,
                              const double *thresholds_host, int T, double *err_dev, int32_t *correct_dev, void *stream);

/* ---- batched synthetic-pair validation (check_val_repeatability, balf/utils/train_utils.py:205-306) -----------------------
 * balf_val_points: the point selection of that loop for P pairs x 2 sides, stream-ordered, nothing read back.  Per side
 *   nms    = the NMS map of the side's score map, no border frame:
 *              BALF_VAL_LEG_GREEDY  get_nms_score_map_from_score_map (repeatability_tools.py:82-100): candidates >= conf_thresh
 *                                   (> 0), nms_fast with dist_thresh = nms_size (<= 16), survivors scattered into a zero map
 *                                   (balf_greedy_nms' kept list; conf_thresh is ignored by the window leg);
 *              BALF_VAL_LEG_WINDOW  apply_nms(prob, nms_size) (:19-23), 1 <= nms_size <= BALF_MAX_NMS_SIZE;
 *   masked = nms * the side's common-region mask (balf_common_region_masks for the pair with border 15, evaluated at the NMS
 *            survivors only, the inverse maps computed on the device in the same operations; a singular h_dst_2_src gives
 *            empty masks);
 *   rows   = get_point_coordinates(masked, num_points = K, 'xysr') (geometry_tools.py:86-125): the first K pixels in RASTER
 *            order with masked >= the K-th largest value of masked.  When that value is <= 0 the threshold is the smallest
 *            positive value (fewer than K positive values: exactly those, count < K), and with no positive value at all it
 *            is 0: the first K raster pixels of the whole map with score 0.
 * prob_src_dev [P,h_src,w_src] / prob_dst_dev [P,h_dst,w_dst] fp32 (scores are probabilities, >= +0), h_dst_2_src_dev [P,9]
 * float64 row-major.  src_pts_dev / dst_pts_dev [P,K,4] float64 rows (x, y, 1.0, score); the destination rows are warped
 * into the source image as balf_apply_homography does (x', y', radius, score).  count_dev [P,2] int32 = rows of (source,
 * destination); rows past the count are 0.  The layout is what balf_repeatability_batch takes (strides 4, count_stride 2).
 * K <= BALF_MAX_TOPK, K <= h * w of both sides (the reference raises IndexError; BALF_ERR_SHAPE), 1 <= P <= 65535; greedy leg:
 * ceil(h / (nms_size + 1)) * ceil(w / (nms_size + 1)) <= BALF_MAX_TOPK (a bound on the points it can keep; BALF_ERR_SHAPE). */
#define BALF_VAL_LEG_GREEDY 0
#define BALF_VAL_LEG_WINDOW 1
size_t balf_val_points_workspace_bytes(int P, int h_src, int w_src, int h_dst, int w_dst, int leg, int nms_size, int K);
int balf_val_points(const float *prob_src_dev, int h_src, int w_src, const float *prob_dst_dev, int h_dst, int w_dst, int P,
                    const double *h_dst_2_src_dev, int leg, float conf_thresh, int nms_size, int K, double *src_pts_dev,
                    double *dst_pts_dev, int32_t *count_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- the resize protocol of the HSequences evaluation (balf/configs/config_hpatches.py: parse_resize_eval_config) -----------
 * balf_resize_repeatability_batch: compute_resize_repeatability (balf/benchmark_test/repeatability_tools.py:516-614) for P
 * independent pairs, stream-ordered, nothing read back.  Rows of src_dev [P,ns_max,src_stride] / dst_dev [P,nd_max,dst_stride]
 * float64; order_xy = 0: a row starts with (row, col, prob), the reference's order (stride >= 3); order_xy = 1: a row is
 * (x, y, radius, score) as the detectors of this library write it (stride >= 4; x = col, y = row, the radius is not read).
 * Pair p's rows start at row p * n_max, its counts are ns_dev[p * count_stride] / nd_dev[p * count_stride] (clamped to
 * [0, n_max]); rows past a count are never read (src_dev / dst_dev may be null when its n_max is 0).  h_dev [P,9] row-major maps source (x, y) to destination (x, y),
 * h_inv_dev [P,9] is its inverse (computed by the caller on the host, np.linalg.inv, as the reference does; nothing is inverted
 * here); shapes_dev [P,4] int32 = (h_src, w_src, h_dst, w_dst).  Per pair:
 *   destination rows: warped with h_inv on (col, row); a row whose warped 0 <= row < h_src and 0 <= col < w_src is kept and
 *                     goes on UNWARPED;
 *   source rows:      warped with h; the WARPED (row, col, prob) goes on when inside (h_dst, w_dst);
 *   select_k_best:    the keep_k_points rows of highest prob of each side (all when fewer).  Ties at the cut: higher prob
 *                     first, then the lower original index (the reference cuts with NumPy's unstable argsort); -0.0 and
 *                     +0.0 are equal probs.  Probs are finite: a NaN prob is outside the contract (its place in the order
 *                     is unspecified);
 *   N1 x N2 Euclidean distances sqrt(dy*dy + dx*dx) (float64, no fused operation), row minima (when N2 != 0) and column minima
 *   (when N1 != 0), count1 / count2 = minima <= distance_thresh, summed in one fixed order (a pair's result does not depend on
 *   P or on its place in the batch).
 * Outputs: rep_dev [P,2] float64 = (repeatability = (count1 + count2) / (N1 + N2) * 100, localization_err = sum1 / (count1 +
 * count2) + sum2 / (count1 + count2)); count1 + count2 == 0 gives (0.0, -1.0).  counts_dev [P,4] int32 = (common_src_num N1,
 * common_dst_num N2, rep_src_num count1, rep_dst_num count2).  The inputs are never written (the reference overwrites the
 * caller's source array with the warped coordinates; that is not reproduced).
 * Limits: 1 <= P <= 65535, ns_max, nd_max <= 65536, 1 <= keep_k_points <= BALF_MAX_TOPK, distance_thresh >= 0 (BALF_ERR_ARG).
 * rr_min_kernel stages 1024 kept rows of the other side at a time in 16 KB of LDS, whatever the counts.
 *
 * balf_resize_crop_u8: ratio_preserving_resize (balf/datasets/dataset_utils.py:15-27) of B uint8 images of DIFFERENT sizes into
 * out_dev [B, target_h, target_w, channels] (channels 1 or 3, interleaved), one launch.  packed_dev holds the images back to
 * back, image b = sizes_dev[b] = (h, w) int32 starting at byte offsets_dev[b] (int64); an image that does not lie inside
 * packed_bytes comes out all zero.  Per image scale = max(target_h / h, target_w / w), new = round_half_even((h, w) * scale)
 * in float64; bilinear resize to `new`, then the centred crop / zero pad: the output pixel (y, x) is the resized pixel
 * (y - top, x - left), top = floor((target_h - new_h) / 2), left = (target_w - new_w) - floor((target_w - new_w) / 2) (the
 * reference hands its four amounts to imgaug's CropAndPad, whose order is top, right, bottom, left), zero where that falls
 * outside the resized image.  The resize is DEFINED here as OpenCV's INTER_LINEAR for uint8 is documented to work (parity with a
 * cv2 build is unpinned): per axis, output coordinate d samples f = float32((d + 0.5) * (n_src / n_new) - 0.5)
 * (float64 product and difference), s = floor(f), f -= s; s < 0 -> (s, f) = (0, 0); s >= n_src - 1 -> (n_src - 1, 0); the
 * second tap is min(s + 1, n_src - 1); weights w0 = rint((1 - f) * 2048), w1 = rint(f * 2048) in float32 (half to even).
 * Horizontal pass S = p[s] * w0 + p[s + 1] * w1 (int32) on the two rows, vertical pass
 * out = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.
 * 1 <= B <= 65535 (BALF_ERR_ARG), target_h, target_w <= 16384 (BALF_ERR_SHAPE).  No workspace. */
size_t balf_resize_repeatability_batch_workspace_bytes(int P, int ns_max, int nd_max, int keep_k_points);
int balf_resize_repeatability_batch(const double *src_dev, const int32_t *ns_dev, int ns_max, int src_stride,
                                    const double *dst_dev, const int32_t *nd_dev, int nd_max, int dst_stride, int count_stride,
                                    int order_xy, int P, const double *h_dev, const double *h_inv_dev,
                                    const int32_t *shapes_dev, int keep_k_points, double distance_thresh, double *rep_dev,
                                    int32_t *counts_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int balf_resize_crop_u8(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev,
                        const int32_t *sizes_dev, int B, int channels, int target_h, int target_w, unsigned char *out_dev,
                        void *stream);

/* ---- synthetic-homography image pairs of the validation task (balf/datasets/COCO.py:42-205; GOPRO inherits it) -----------
 * balf_synth_pairs: what the reference's loader computes per pair AFTER the homography and the two windows are drawn (host:
 * balf_amd/datasets/dataset_utils.py: sample_pair_geometry), for P pairs, stream-ordered, nothing read back, capturable.  Only
 * the patch x patch windows are computed; the full warped image and the full-size heat maps are never formed.
 * Inputs: packed_dev the uint8 RGB-interleaved source images back to back, image p = sizes_dev[p] = (h, w) int32 at byte
 * offsets_dev[p] (int64), as balf_resize_crop_u8 takes them (pairs may share an image); inv_h_dev [P,9] float64 row-major, the
 * matrix the reference hands to cv2.warpPerspective (COCO.py:67-68,75); win_src_dev / win_dst_dev [P,2] int32 = (top row, left
 * column) of the two windows in full-image coordinates; pts_dev [pts_total,3] float32 label rows (x, y, prob), pair p's rows
 * are pts_offsets_dev[p] .. pts_offsets_dev[p + 1] (int32, P + 1 entries; a range outside [0, pts_total] counts as empty).
 * Outputs (float32): img_src_dev / img_dst_dev [P,3,patch,patch] planar, heat_src_dev / heat_dst_dev [P,1,patch,patch],
 * dst_max_dev [P] int32.  Per pair:
 *   source patch       (float)((double)byte / 255.0) of the source window (the reference divides in float64, then narrows).
 *   destination patch  cv2.warpPerspective(src, inv_h, (w, h)) with default flags (bilinear, constant-zero border) for 8-bit
 *                      3-channel data at the destination window's pixels, DEFINED here as OpenCV's 8-bit INTER_LINEAR remap is
 *                      documented to work (parity with a cv2 build is unpinned): output pixel (x, y) samples
 *                      M (x, y, 1), M = the closed-form inverse of inv_h, exactly as balf_common_region_masks does (one shared
 *                      device function): X = M0 x + M1 y + M2 etc. in float64 without fused operations, 32 / W (0 for W = 0),
 *                      clamped to the int range, rounded half to even; tap = value >> 5, fractions fx, fy = value & 31.
 *                      Integer weights (32-fx)(32-fy)32, fx(32-fy)32, (32-fx)fy 32, fx fy 32 (sum 32768); a tap outside the
 *                      source image contributes 0; byte = (sum + 16384) >> 15; then / 255 as above.  At a pixel where W is
 *                      exactly 0 both coordinates are 0: the tap is source pixel (0, 0).  A singular inv_h (the determinant
 *                      of the closed form is exactly 0, e.g. a zero row) gives an all-zero patch and dst_max = 0; the pair's
 *                      source patch and both heat maps are computed as for any other pair (the label warp divides by its
 *                      own float32 denominator, below), and the other pairs of the call are not affected.
 *   dst_max            the largest byte of the destination patch (0: an all-black patch).  The reference redraws a homography
 *                      whose WHOLE warped image is black (COCO.py:77); that image is never formed here, nothing is redrawn, and
 *                      the caller gets this value instead.
 *   labels             select_k_best (dataset_utils.py:277-286): the top_k rows of largest prob; top_k == 0 or fewer rows than
 *                      top_k keep all.  Ties at the cut keep the LOWER row index (the reference cuts with NumPy's unstable
 *                      argsort: arbitrary there).  Kept points are truncated to integers (xi, yi).
 *   source heat map    1.0 at (yi, xi) of each kept point inside the source window, 0 elsewhere (labels_to_heatmap, :288-292;
 *                      a point outside the image is dropped, where NumPy would wrap a negative index or raise).
 *   dest. heat map     apply_homography_to_source_labels_torch as it returns (:200-219; its bilinear labels are discarded by
 *                      the reference and not computed): (xi, yi) warped with inv_h NARROWED TO float32 in float32 arithmetic
 *                      without fused operations, x' = ((h0 xi + h1 yi) + h2) / ((h6 xi + h7 yi) + h8); kept where 0 <= x' <=
 *                      w - 1 and 0 <= y' <= h - 1 of the FULL image (both ends included; a denominator of exactly 0 gives an
 *                      infinity or a NaN, which is dropped here); rounded half to even; 1.0 where the rounded point lies
 *                      inside the destination window, 0 elsewhere.
 * The heat maps are zeroed by the call itself.  An image that does not lie inside packed_bytes gives all-zero outputs; a window
 * that leaves its image is read clamped (source) / evaluated where it lies (destination); both report dst_max = -1 (the
 * windows live on the device, so the host cannot refuse them).
 * Limits: 1 <= P <= 65535, patch >= 1, top_k >= 0, pts_total >= 0 (BALF_ERR_ARG); patch <= 16384 (BALF_ERR_SHAPE).  pts_dev
 * may be null when pts_total is 0.  The workspace holds one int per 1024 output pixels and pair. */
size_t balf_synth_pairs_workspace_bytes(int P, int patch);
int balf_synth_pairs(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev,
                     const int32_t *sizes_dev, int P, const double *inv_h_dev, const int32_t *win_src_dev,
                     const int32_t *win_dst_dev, const float *pts_dev, int pts_total, const int32_t *pts_offsets_dev,
                     int top_k, int patch, float *img_src_dev, float *img_dst_dev, float *heat_src_dev, float *heat_dst_dev,
                     int32_t *dst_max_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- the training task's pairs: photometric distortion (balf/datasets/dataset_utils.py:76-134, COCO.py:70-75) -------------
 * The reference's training loader warps bgr_photometric_to_rgb(src_BGR), not the image itself.  The random draws stay on the
 * host (balf_amd/datasets/dataset_utils.py: sample_photometric); per image / pair the device takes params [5] float64 =
 * (delta_b, alpha1, sat, hue, alpha2) and perm int32, a row of the reference's perms table ((0,1,2), (0,2,1), (1,0,2), (1,2,0),
 * (2,0,1), (2,1,0)).  A branch of bgr_distorsion that did not fire is its neutral value -- delta_b = 0, alpha = 1, sat = 1,
 * hue = 0, perm = 0 --, which makes the step the identity bit for bit, so there are no flags.
 * The two colour conversions are DEFINED here by OpenCV's scalar 8-bit code (RGB2HSV_b with hrange 180, HSV2RGB_b through its
 * float32 path); parity with a cv2 build is UNPINNED (no cv2 where this library is built), as for the warp and
 * the resize.  Per pixel, from bytes (b, g, r):
 *   1  x = (double)byte + delta_b, clamped to [0, 255] (x > 255 -> 255, then x < 0 -> 0); x *= alpha1, clamped; truncated.
 *   2  v = max, vmin = min, diff = v - vmin; sdiv[i] = rint((255 << 12) / (double)i), hdiv[i] = rint((180 << 12) / (6.0 * i)),
 *      sdiv[0] = hdiv[0] = 0; S = (diff * sdiv[v] + 2048) >> 12; h = (v == r) ? g - b : (v == g) ? b - r + 2 diff : r - g +
 *      4 diff (in this order when channels tie); H = (h * hdiv[diff] + 2048) >> 12 (arithmetic shift, int32), H += 180 if H < 0.
 *   3  S = trunc(clamp((double)S * sat)).
 *   4  x = (double)H + hue; x -= 360 if x > 360; x += 360 if x < 0; the byte is (int32)x & 255.  This is what the reference's
 *      astype(np.uint8) gives on x86-64: 324..359 become 68..103, a hue jump the reference really makes; it is reproduced.
 *   5  s = S * (1.f / 255.f), vv = V * (1.f / 255.f) in float32 without fused operations.  S == 0: b = g = r = vv.  Otherwise
 *      hh = H * (6.f / 180.f), hh -= 6.f if hh >= 6.f, sector = floor(hh), f = hh - sector, tab = {vv, vv (1 - s),
 *      vv (1 - s f), vv (1 - s (1 - f))}, (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector]; the byte
 *      is rint(x * 255.f) (half to even) saturated to [0, 255].
 *   6  x = (double)byte * alpha2, clamped, truncated.
 *   7  out_bgr[k] = bgr[perms[perm][k]].
 * Finite parameters are the contract; whatever bits they hold, every table index is a byte, so no read leaves its table.
 *
 * balf_photometric_u8: steps 1-7 on B whole 3-channel interleaved uint8 images, one launch, no workspace, stream-ordered,
 * capturable.  The images are packed as balf_resize_crop_u8 takes them (offsets_dev [B] int64, sizes_dev [B,2] int32 (h, w));
 * out_dev has the layout and the offsets of packed_dev (it may BE packed_dev).  params_dev [B,5] float64, perm_dev [B] int32.
 * blue_idx 0: the pixels are B, G, R; 2: R, G, B (b = px[blue_idx], r = px[2 - blue_idx]); the output keeps the input's order.
 * An image that does not lie inside packed_bytes is not written; a perm outside 0..5 writes a black image.
 * 1 <= B <= 65535, blue_idx in {0, 2} (BALF_ERR_ARG).
 *
 * balf_synth_train_pairs: balf_synth_pairs for the training task: the same arguments, then params_dev [P,5] and perm_dev [P];
 * the same workspace (balf_synth_pairs_workspace_bytes), limits and errors, and the same outputs except the destination patch
 * and dst_max.  The packed images are RGB, as for balf_synth_pairs, and the destination patch is the warp of
 * bgr_photometric_to_rgb(image) -- the distortion reads blue from px[2] and writes in the input's order, blue_idx = 2 above.
 * The distorted image is never formed: each of the four taps of an output pixel is distorted, all three channels, before the
 * integer interpolation.  A tap outside the image contributes 0, NOT the distortion of a black pixel: the reference pads the
 * already distorted image with zeros.  The source patch is the undistorted image; dst_max is the largest byte of the
 * distorted, warped patch.  A perm outside 0..5 gives an all-zero destination patch and dst_max = -1; the pair's other
 * outputs and the other pairs of the call are as for any pair.  The destination patch, both heat maps and dst_max equal, bit
 * for bit, those of balf_photometric_u8 (blue_idx 2) followed by balf_synth_pairs on its output (whose SOURCE patch is cut from
 * the distorted image, which is not the training task's). */
int balf_photometric_u8(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev,
                        const int32_t *sizes_dev, int B, const double *params_dev, const int32_t *perm_dev, int blue_idx,
                        unsigned char *out_dev, void *stream);
int balf_synth_train_pairs(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev,
                           const int32_t *sizes_dev, int P, const double *inv_h_dev, const int32_t *win_src_dev,
                           const int32_t *win_dst_dev, const float *pts_dev, int pts_total, const int32_t *pts_offsets_dev,
                           int top_k, int patch, float *img_src_dev, float *img_dst_dev, float *heat_src_dev,
                           float *heat_dst_dev, int32_t *dst_max_dev, void *workspace_dev, size_t workspace_bytes,
                           const double *params_dev, const int32_t *perm_dev, void *stream);

/* ---- detector (anchor) loss: labels, masked cross-entropy and its gradient (balf/loss/loss_function.py:7-26) ------------
 * balf_detector_loss: the reference's detector_loss for grid_size 8 (the 65-channel head, the only one arch.py supports; the
 * reference's train_model passes grid_size=16, which its own 65-channel head cannot satisfy), stream-ordered, nothing read
 * back, capturable, statement by statement.  A cell is one element of the [Hc,Wc] plane; n = Hc * Wc.
 * Inputs (float32): logits_dev [B,65,Hc,Wc] as balf_forward writes them; keypoint_map_dev [B,1,8Hc,8Wc]; valid_mask_dev
 * [B,1,8Hc,8Wc] or NULL = all ones (loss_function.py:16; bit-identical to a mask of ones); noise_dev [B,65,Hc,Wc], the random
 * tie-break the reference draws itself (:13), or NULL = no noise.  The arithmetic is the library's, the random numbers the caller's.
 *   labels (:8-13)    channel c = dy * 8 + dx of a cell is pixel (8y + dy, 8x + dx) (tensor_op.pixel_shuffle_inv with one input
 *                     channel).  v_c = fl32(fl32(2 * kp) + noise[c]) for c < 64, the dustbin v_64 = fl32(1 + noise[64]); label =
 *                     the FIRST index of the maximum (torch.argmax).  One exact doubling and one rounding per value: labels are
 *                     bit-identical to the reference for every finite input.  Without noise the lowest channel among several
 *                     key points of a cell wins, a key-point value of 0.5 ties the dustbin and wins, and an empty cell gets 64.
 *                     NaN inputs are outside the contract.
 *   cell mask (:16-18) vm = the product of the cell's 64 mask values, multiplied in channel order in float32: exact in any
 *                     order for masks of zeros and ones, which is the contract; for other values the order is this one and
 *                     parity with torch.prod is unpinned.
 *   cross-entropy (:21) ce = lse(logits[:, cell]) - logits[label, cell]; the log-sum-exp subtracts the maximum first (a logit of
 *                     100 does not overflow): float32 exponentials of (logit - max), summed and finished in float64.
 *   per image (:23)   num_b = sum(ce * vm), den_b = sum(fl32(vm + 1e-6f)), both in float64 in ONE fixed order that depends on
 *                     (Hc, Wc) alone -- no floating-point atomics; an image's value does not depend on B or on its place in
 *                     the batch.  per_image[b] = fl32(num_b / den_b); a fully masked image gives 0 (den = n * 1e-6).
 *   loss (:24)        fl32(mean_b(num_b / den_b)), the mean in float64 in index order.
 *   gradient          dlogits[b,c,cell] = fl32((softmax_c - [c == label]) * vm / (den_b * B)): d loss / d logits.
 * Outputs: loss_dev [1] float32; per_image_dev [B] float32, labels_dev [B,Hc,Wc] int32, dlogits_dev [B,65,Hc,Wc] float32, each
 * may be NULL and is then neither computed nor written.  The results do not depend on which outputs are requested.
 * Four launches whatever is requested (cell masks and denominator partial sums; denominators; the pass over the logits, which
 * are read ONCE and stay in registers between the log-sum-exp and the gradient; the per-image ratios and the loss).  Every
 * word of the workspace that is read has been written by the same call; nothing needs clearing.  keypoint_map_dev and
 * valid_mask_dev are read with 16-byte loads when they are 16-byte aligned, with 4-byte loads otherwise (same results).
 * Limits: 1 <= B <= 65535 (BALF_ERR_ARG); Hc, Wc >= 1 (BALF_ERR_ARG), Hc * Wc <= 2^24 (BALF_ERR_SHAPE); logits_dev,
 * keypoint_map_dev, loss_dev and workspace_dev must not be NULL and workspace_dev must be 8-byte aligned (BALF_ERR_ARG); a workspace smaller than
 * balf_detector_loss_workspace_bytes(B, Hc, Wc) (0 for sizes outside the limits) gives BALF_ERR_WORKSPACE. */
size_t balf_detector_loss_workspace_bytes(int B, int Hc, int Wc);
int balf_detector_loss(const float *logits_dev, const float *keypoint_map_dev, const float *valid_mask_dev,
                       const float *noise_dev, int B, int Hc, int Wc, float *loss_dev, float *per_image_dev,
                       int32_t *labels_dev, float *dlogits_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- the trainable tail of the detector: training-mode head and its backward ------------------------------
 * down4.conv2 (Linear 256 -> 256) -> ReLU -> detector_head.dense (Linear 256 -> 65) -> detector_head.norm (BatchNorm2d with
 * BATCH statistics), and the backward from dlogits (balf_detector_loss writes it) to the six parameter gradients and to the
 * gradient of the stage-4 activation x2.  N = B * Hc * Wc pixels.  X = x2_dev [N,256] float32 NHWC, what
 * balf_forward_stage_view(stage = 4) writes.  The parameters are plain float32 device tensors in PyTorch layout, NOT the packed
 * blob (they change every step): w2_dev [256,256], b2_dev [256], wd_dev [65,256], bd_dev [65], gamma_dev, beta_dev [65].
 *   forward    h = X W2^T + b2;  a = max(h, 0);  z = a Wd^T + bd  [N,65]
 *              mu_c = mean_N z, var_c = the biased variance, both from float64 sums of z and z * z;  r_c = 1 / sqrt(var_c + eps)
 *              in float64;  xhat = fl32((z - mu) * r) (float64 inside);  logits[b,c,y,x] = fma(gamma_c, xhat, beta_c), NCHW
 *              [B,65,Hc,Wc] as balf_forward writes them.
 *              prob_dev (NULL ok) [B,8Hc,8Wc]: softmax over the 65 logits (maximum taken out), dustbin dropped, pixel-shuffled.
 *              running_mean_dev / running_var_dev (each NULL ok) [65]: rm <- (1 - m) rm + m mu, rv <- (1 - m) rv + m var N / (N - 1),
 *              evaluated in float64, m = momentum.
 *              use_stats = 1: normalise with stats_in_dev [2,65] (mean, then variance) instead of the batch's -- the eval mode of
 *              the same kernels: no statistics pass, no running-statistics update, and no backward is defined for it.
 *   backward   g = dlogits_dev [B,65,Hc,Wc]:  dbeta = sum_N g,  dgamma = sum_N g xhat  (float64, xhat = (z - mu) r kept in float64:
 *              the three terms of dz cancel almost completely when N is small),
 *              dz = gamma r (g - dbeta / N - xhat dgamma / N)  (float64 inside, stored as float32)
 *              dWd = dz^T a,  dbd = sum dz,  da = dz Wd,  dh = da [h > 0] (0 at h == 0, as torch),  dW2 = dh^T X,  db2 = sum dh,
 *              dx2 = dh W2  (dx2_dev NULL ok).
 * saved_dev: an opaque caller-owned block of balf_head_train_saved_bytes(N) bytes that the forward writes and the backward of
 * the same (B, Hc, Wc) reads: a [N,256], z itself, channel-major [65,N] (never recomputed from the logits: gamma_c may be 0),
 * and mu, r as float64.
 * Arithmetic: the six matrix products run on v_mfma_f32_16x16x4_f32, exact float32 fma chains with k ascending; the 65-wide
 * side is padded inside the kernel (pad elements are never loaded, never stored, and enter a tile as 0).  No floating-point
 * atomics: the statistics, dbeta, dgamma and dbd are float64 partial sums per workgroup of 1024 pixels, added per channel by one
 * wave in a fixed order; db2 likewise over blocks of rows; dW2 and dWd are summed over S = ceil(N / rows) slices of the pixels,
 * rows = 256 * ceil(ceil(N / 256) / 64) (S <= 64), each slice an fma chain into its own slab of the workspace, the slabs added
 * in float64 in slice order.  Every order is a function of N alone: two calls on the same input give bit-identical outputs.
 * An output that is not requested (prob, the running statistics, dx2) is neither computed nor written, and the others do not
 * change with that.  Stream-ordered, nothing synchronised or read back, capturable; every word of the workspace and of saved
 * that is read was written before, by the same call or (saved) by the forward.
 * Launches: forward 5 (4 with use_stats), backward 12 (13 with dx2).
 * Limits: 1 <= B <= 65535, Hc, Wc >= 1 and N >= 2 (BALF_ERR_ARG: one value per channel has no variance, torch raises there
 * too); N <= 2^24 (BALF_ERR_SHAPE); the required pointers (everything not marked NULL ok; stats_in_dev with use_stats) must not
 * be NULL, saved_dev and workspace_dev must be 8-byte aligned, eps >= 0 (BALF_ERR_ARG); a workspace smaller than
 * balf_head_train_workspace_bytes(N) gives BALF_ERR_WORKSPACE.  Both size queries return 0 for N outside [2, 2^24]. */
size_t balf_head_train_workspace_bytes(long N);
size_t balf_head_train_saved_bytes(long N);
int balf_head_train_forward(const float *x2_dev, const float *w2_dev, const float *b2_dev, const float *wd_dev,
                            const float *bd_dev, const float *gamma_dev, const float *beta_dev, int B, int Hc, int Wc, double eps,
                            int use_stats, const float *stats_in_dev, float *logits_dev, float *prob_dev, float *running_mean_dev,
                            float *running_var_dev, double momentum, void *saved_dev, void *workspace_dev, size_t workspace_bytes,
                            void *stream);
int balf_head_train_backward(const float *dlogits_dev, const float *x2_dev, const float *w2_dev, const float *wd_dev,
                             const float *gamma_dev, const void *saved_dev, int B, int Hc, int Wc, float *dw2_dev, float *db2_dev,
                             float *dwd_dev, float *dbd_dev, float *dgamma_dev, float *dbeta_dev, float *dx2_dev,
                             void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- stage 4's channel-attention block (RCAB) in training form, and its backward ---------------------------
 * The block directly above x2: LayerNorm -> conv1 (Linear 256 -> 256) -> LeakyReLU(0.2) -> conv2 (Linear 256 -> 256) ->
 * squeeze-excite scale, plus both shortcuts.  N = B * Hc * Wc pixels, i = the image of pixel p.  y_dev [N,256] is the block's
 * input, r_dev [N,256] = y + x0 with x0 = relu(down4.conv.0(.)) the long shortcut (balf_forward_rcab_inputs writes both).  The
 * ten parameters under down4.residual_channel_attention_block. are plain float32 device tensors in PyTorch layout: ln_g, ln_b
 * [256] (norm), wc1 [256,256], bc1 [256] (conv1), wc2, bc2 (conv2), ws0 [64,256], bs0 [64] (calayer.excite.0), ws2 [256,64],
 * bs2 [256] (calayer.excite.2).
 *   forward    mean, var over the 256 channels of a pixel, the variance from the centred values; rstd = 1 / sqrt(var + 1e-5);
 *              xhat = (y - mean) rstd;  n = fma(xhat, ln_g, ln_b);  h = n wc1^T + bc1;  a = h > 0 ? h : 0.2 h;  t = a wc2^T + bc2;
 *              m_i = mean of t over the pixels of image i;  e_i = relu(m_i ws0^T + bs0);  s_i = sigmoid(e_i ws2^T + bs2)  (float64);
 *              x2 = fma(t, fl32(s_i), r)  -- the formula of the inference forward.
 *   backward   g = dx2_dev [N,256]:  ds_i = sum_p g t;  dq = ds s (1 - s);  dws2 = sum_i dq_i^T e_i;  dbs2 = sum_i dq_i;
 *              de = (dq ws2) [e > 0];  dws0 = sum_i de_i^T m_i;  dbs0 = sum_i de_i;  dm = de ws0  (all float64, images in order);
 *              dt = fma(g, fl32(s_i), fl32(dm_i / (Hc Wc)));  dwc2 = dt^T a;  dbc2 = sum_p dt;  da = dt wc2;
 *              dh = da (a > 0 ? 1 : 0.2)  (0.2 at h == 0, as torch);  dwc1 = dh^T n;  dbc1 = sum_p dh;  dn = dh wc1;
 *              dln_g = sum_p dn xhat;  dln_b = sum_p dn;  u = dn ln_g;
 *              dy = g + rstd (u - mean_c u - xhat mean_c(u xhat))  (dy_dev NULL ok) -- the gradient at the block's input, its own
 *              shortcut included.  The long shortcut's gradient is g itself and is not written.
 * saved_dev: an opaque caller-owned block of balf_rcab_train_saved_bytes bytes that the forward writes and the backward of the
 * same (B, Hc, Wc) reads: n, a, t [N,256], (mean, rstd) per pixel, m [256], e [64], s [256] per image as float64, and s once more
 * as float32 (the factor of x2).  The backward recomputes xhat from y and the saved (mean, rstd) with the forward's operations
 * (ln_g may be 0).
 * Arithmetic: the six 256 x 256 products run on v_mfma_f32_16x16x4_f32 (the GEMM of the head, train_gemm.h), dwc1 / dwc2 over
 * S = ceil(N / rows) slices of the pixels with a float64 slab sum, as dW2 of the head.  A LayerNorm row is one wave, four
 * channels per lane, every channel sum (v0 + v1) + (v2 + v3) and then the xor butterfly.  Every sum over pixels (m, ds, dbc1,
 * dbc2, dln_g, dln_b) is made of float64 per-workgroup partials added in one fixed order; m and ds per image, over row blocks of
 * THAT image (max(64, ceil(Hc Wc / 1024)) rows each), so that no partial mixes two images.  No floating-point atomics; every
 * order is a function of (B, Hc, Wc) alone: two calls on the same input give bit-identical outputs.  dy, when not requested, is
 * neither computed nor written and the other outputs do not change.  Stream-ordered, nothing synchronised or read back,
 * capturable; every word of the workspace and of saved that is read was written before.
 * Launches: forward 6, backward 16.
 * Limits: 1 <= B <= 65535, Hc, Wc >= 1, N >= 2 (BALF_ERR_ARG), N <= 2^24 (BALF_ERR_SHAPE); the required pointers must not be
 * NULL; y_dev, r_dev, x2_dev, ln_g_dev, ln_b_dev, saved_dev and workspace_dev must be 16-byte aligned (dx2_dev and dy_dev need 4)
 * (BALF_ERR_ARG); a workspace smaller than balf_rcab_train_workspace_bytes gives BALF_ERR_WORKSPACE.  Both size queries return 0
 * outside these limits. */
size_t balf_rcab_train_workspace_bytes(int B, int Hc, int Wc);
size_t balf_rcab_train_saved_bytes(int B, int Hc, int Wc);
int balf_rcab_train_forward(const float *y_dev, const float *r_dev, const float *ln_g_dev, const float *ln_b_dev,
                            const float *wc1_dev, const float *bc1_dev, const float *wc2_dev, const float *bc2_dev,
                            const float *ws0_dev, const float *bs0_dev, const float *ws2_dev, const float *bs2_dev, int B, int Hc,
                            int Wc, float *x2_dev, void *saved_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int balf_rcab_train_backward(const float *dx2_dev, const float *y_dev, const float *ln_g_dev, const float *wc1_dev,
                             const float *wc2_dev, const float *ws0_dev, const float *ws2_dev, const void *saved_dev, int B, int Hc,
                             int Wc, float *dln_g_dev, float *dln_b_dev, float *dwc1_dev, float *dbc1_dev, float *dwc2_dev,
                             float *dbc2_dev, float *dws0_dev, float *dbs0_dev, float *dws2_dev, float *dbs2_dev, float *dy_dev,
                             void *workspace_dev, size_t workspace_bytes, void *stream);
/* The same block at C channels, C = 256 (stage 4; what the two functions above call) or 128 (stage 3's, under
 * down3.residual_channel_attention_block.); any other C gives BALF_ERR_SHAPE.  Read C for 256 and C / 4 for 64 in everything
 * above.  At C = 128 a LayerNorm row is a half-wave, two pixels per wave, the butterfly 16..1 inside the half-wave; the column
 * kernels run C threads per workgroup.  The sizes of saved_dev and workspace_dev at C come from balf_train_unit_sizes. */
int balf_rcab_train_forward_c(const float *y_dev, const float *r_dev, const float *ln_g_dev, const float *ln_b_dev,
                              const float *wc1_dev, const float *bc1_dev, const float *wc2_dev, const float *bc2_dev,
                              const float *ws0_dev, const float *bs0_dev, const float *ws2_dev, const float *bs2_dev, int B, int Hc,
                              int Wc, int C, float *x2_dev, void *saved_dev, void *workspace_dev, size_t workspace_bytes,
                              void *stream);
int balf_rcab_train_backward_c(const float *dx2_dev, const float *y_dev, const float *ln_g_dev, const float *wc1_dev,
                               const float *wc2_dev, const float *ws0_dev, const float *ws2_dev, const void *saved_dev, int B, int Hc,
                               int Wc, int C, float *dln_g_dev, float *dln_b_dev, float *dwc1_dev, float *dbc1_dev, float *dwc2_dev,
                               float *dbc2_dev, float *dws0_dev, float *dbs0_dev, float *dws2_dev, float *dbs2_dev, float *dy_dev,
                               void *workspace_dev, size_t workspace_bytes, void *stream);
/* After a forward whose last micro-batch of B images is resident in workspace_dev (the rules and error codes of
 * balf_forward_stage_view): r_dev [B,Hp/8,Wp/8,256] = the forward's own y + x0, copied; x0 = relu(x3 W^T + b) computed again from
 * the resident stage-3 output (view 3, de-fragmented on the split-f16 path) with the training GEMM and conv0_w_dev [256,128],
 * conv0_b_dev [256] = down4.conv.0; y_dev = r - x0.  y therefore carries one more rounding of r and the difference of the two
 * evaluations of x0.  The forward's kernels and buffers are only read; the two outputs serve as scratch, nothing is allocated. */
int balf_forward_rcab_inputs(int precision, const void *workspace_dev, size_t workspace_bytes, int B, int Hp, int Wp,
                             const float *conv0_w_dev, const float *conv0_b_dev, float *y_dev, float *r_dev, void *stream);

/* ---- stage 4's multi-axis gated-MLP layer in training form, and its backward ------------------------------
 * The layer directly above the RCAB: down4.residual_split_head_multi_axis_gmlp_layer.  N = B * Hc * Wc pixels; x0_dev [N,256]
 * float32 NHWC is its input (relu(down4.conv.0(.)), balf_forward_gmlp_input writes it), y_dev [N,256] its output, the y of
 * balf_rcab_train_forward.
 *   forward    n0 = LN(x0);  h0 = n0 W1^T + b1 [N,512];  (u, v) = the halves of gelu(h0), gelu(h) = h Phi(h), the exact erf form;
 *              branch(z, map):  nb = LN_b(z);  hb = nb Wb1^T + bb1 [N,512];  (a, c) = the halves of gelu(hb);  cn = LN_g(c);
 *                               mix[p][ch] = sum_q Wt[p][q] cn[q][ch] + bt[p] over the 64 tokens of one group, per channel;
 *                               z' = z + (a * (mix + 1)) Wb2^T + bb2;
 *              u' = branch(u, grid);  v' = branch(v, block);  y = cat(u', v') W2^T + b2 + x0.
 *              Grid map: token = which of the 8 x 8 image regions of (Hc / 8) x (Wc / 8) pixels, group = (image, position inside
 *              the region).  Block map: token = position inside a contiguous 8 x 8 block, group = (image, block).  Tokens count
 *              row-major, 8 * row + column.  Every LN is over the 256 channels of a pixel, eps = 1e-5, as the RCAB's.
 *   backward   g = dy_dev [N,256]:  db2 = sum g;  dW2 = g^T cat;  dcat = g W2;  per branch, dz' = its half of dcat:
 *              dbb2 = sum dz';  dWb2 = dz'^T (a (mix + 1));  dgated = dz' Wb2;  da = dgated (mix + 1);  dmix = dgated a;
 *              dbt[p] = sum over groups and channels of dmix;  dWt[p][q] = sum over groups and channels of dmix[p] cn[q];
 *              dcn[q] = sum_p Wt[p][q] dmix[p];  dc = LN_g'(dcn) (with dLN_g's gain and bias);  dhb = (da, dc) gelu'(hb), gelu'(h) =
 *              Phi(h) + h phi(h) from the saved pre-activation;  dbb1 = sum dhb;  dWb1 = dhb^T nb;  dnb = dhb Wb1;
 *              dz = dz' + LN_b'(dnb);  dh0 = (du, dv) gelu'(h0);  db1 = sum dh0;  dW1 = dh0^T n0;  dn0 = dh0 W1;
 *              dx0 = g + LN'(dn0)  (dx0_dev NULL ok) -- the gradient at the layer's input through the layer, its own shortcut
 *              included.  x0 also feeds the RCAB's long shortcut; that addend (the dx2 of balf_rcab_train_backward) is the caller's.
 * params / grads: HOST arrays of 26 device pointers, float32 tensors in PyTorch layout, in this order (names under
 * down4.residual_split_head_multi_axis_gmlp_layer.):
 *    0 norm.weight [256]            1 norm.bias [256]            2 dense1.weight [512,256]     3 dense1.bias [512]
 *    for L = grid_gmlp_layer (U = grid_gating_unit) at 4 .. 13, then L = block_gmlp_layer (U = block_gating_unit) at 14 .. 23:
 *    +0 L.norm.weight [256]         +1 L.norm.bias [256]         +2 L.dense1.weight [512,256]  +3 L.dense1.bias [512]
 *    +4 L.U.norm.weight [256]       +5 L.U.norm.bias [256]       +6 L.U.dense.weight [64,64]   +7 L.U.dense.bias [64]
 *    +8 L.dense2.weight [256,256]   +9 L.dense2.bias [256]
 *   24 dense2.weight [256,512]     25 dense2.bias [256]
 * saved_dev: an opaque caller-owned block of balf_gmlp_train_saved_bytes bytes that the forward writes and the backward of the
 * same (B, Hc, Wc) reads: n0, h0, gelu(h0), cat, the (mean, rstd) of every LN, and per branch nb, hb, gelu(hb), cn, mix + 1 and
 * a (mix + 1).  Every xhat is recomputed from the LN's input and the saved (mean, rstd) with the forward's operations.
 * Arithmetic: every product along the channels runs on v_mfma_f32_16x16x4_f32 through the GEMM of the head (train_gemm.h), the
 * weight gradients over S = ceil(N / rows) slices of the pixels with a float64 slab sum.  The token mix and dcn are 64 x 64 MFMA
 * products per group, gathered through the map, the summed token ascending.  dWt / dbt: an MFMA chain over 64 channels per wave
 * and group, the groups of a workgroup (ceil(N / 64 / 256) each) added in float64, then the wave partials in one fixed order.
 * Every sum over pixels is made of float64 per-workgroup partials added in one fixed order.  No floating-point atomics; every
 * order is a function of (B, Hc, Wc) alone: two calls on the same input give bit-identical outputs.  dx0, when not requested, is
 * neither computed nor written and the other outputs do not change.  Stream-ordered, nothing synchronised or read back,
 * capturable; every word of the workspace and of saved that is read was written before.
 * Launches: forward 13, backward 51.
 * Limits: 1 <= B <= 65535, Hc, Wc >= 1 (BALF_ERR_ARG); Hc and Wc multiples of 8, N <= 2^24 (BALF_ERR_SHAPE); the required
 * pointers, the two arrays and their 26 entries must not be NULL; x0_dev, y_dev, dy_dev, dx0_dev, the parameters, saved_dev and
 * workspace_dev must be 16-byte aligned (BALF_ERR_ARG); a workspace smaller than balf_gmlp_train_workspace_bytes gives
 * BALF_ERR_WORKSPACE.  Both size queries return 0 outside these limits. */
size_t balf_gmlp_train_workspace_bytes(int B, int Hc, int Wc);
size_t balf_gmlp_train_saved_bytes(int B, int Hc, int Wc);
int balf_gmlp_train_forward(const float *x0_dev, const float *const *params, int B, int Hc, int Wc, float *y_dev, void *saved_dev,
                            void *workspace_dev, size_t workspace_bytes, void *stream);
int balf_gmlp_train_backward(const float *dy_dev, const float *x0_dev, const float *const *params, const void *saved_dev, int B,
                             int Hc, int Wc, float *const *grads, float *dx0_dev, void *workspace_dev, size_t workspace_bytes,
                             void *stream);
/* The same layer at C channels, C = 256 (stage 4; what the two functions above call) or 128 (stage 3's, under
 * down3.residual_split_head_multi_axis_gmlp_layer.); any other C gives BALF_ERR_SHAPE.  Read C for 256 and 2C for 512 in
 * everything above; the token matrices stay [64,64].  At C = 128 the token-mix kernels run two waves per group (wave w owns
 * channels 64 w .. 64 w + 63 as before), so dWt / dbt have 2 wave partials per workgroup instead of 4, added in the same fixed
 * order.  The sizes of saved_dev and workspace_dev at C come from balf_train_unit_sizes. */
int balf_gmlp_train_forward_c(const float *x0_dev, const float *const *params, int B, int Hc, int Wc, int C, float *y_dev,
                              void *saved_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int balf_gmlp_train_backward_c(const float *dy_dev, const float *x0_dev, const float *const *params, const void *saved_dev, int B,
                               int Hc, int Wc, int C, float *const *grads, float *dx0_dev, void *workspace_dev,
                               size_t workspace_bytes, void *stream);
/* After a forward whose last micro-batch of B images is resident in workspace_dev (the rules and error codes of
 * balf_forward_stage_view): x0_dev [B,Hp/8,Wp/8,256] = relu(x3 W^T + b), computed from the resident stage-3 output with the
 * training GEMM exactly as balf_forward_rcab_inputs computes it (the same bits).  scratch_dev: B * Hp/8 * Wp/8 * 128 floats for the
 * de-fragmented stage-3 view of the split-f16 path (NULL ok with BALF_PREC_FP32). */
int balf_forward_gmlp_input(int precision, const void *workspace_dev, size_t workspace_bytes, int B, int Hp, int Wp,
                            const float *conv0_w_dev, const float *conv0_b_dev, float *x0_dev, float *scratch_dev, void *stream);

/* ---- the first layer of a Down stage in training form, and its backward --------------------------------------
 * A per-pixel Linear c_in -> c_out = 2 c_in followed by a ReLU: down4.conv.0 at c_in = 128 (its output is the x0 of
 * balf_forward_gmlp_input), the same layer of stages 3 and 2 at c_in = 64 and 32.  N pixels; x_dev [N,c_in], w_dev [c_out,c_in]
 * (PyTorch layout), b_dev [c_out], y_dev [N,c_out], g_dev [N,c_out] the TOTAL gradient at y, all float32.
 *   forward    y = relu(x w^T + b): the GEMM of the head (train_gemm.h) on v_mfma_f32_16x16x4_f32, k ascending, launched exactly as
 *              balf_forward_gmlp_input launches it -- at c_in = 128 the same bits as its x0 from the same x.
 *   backward   gm = y > 0 ? g : 0, the derivative from the OUTPUT as torch's threshold_backward: a select, so whatever g holds
 *              under a dead unit (huge, non-finite) gives 0, and the derivative at exactly 0 is 0;
 *              db[o] = sum_p gm[p,o];  dw[o,k] = sum_p gm[p,o] x[p,k];  dx = gm w  (dx_dev NULL ok: then it is neither computed
 *              nor written and no other output changes).
 * db: float64 per-workgroup column partials, made in the pass that makes gm, added by one wave in a fixed order.  dw: S =
 * ceil(N / rows) slices of the pixels, each an MFMA chain, the slabs added in float64 in slice order.  No floating-point atomics;
 * every order is a function of (N, c_in) alone: two calls on the same input give bit-identical outputs.  Stream-ordered, nothing
 * synchronised, allocated or read back, capturable; every word of the workspace that is read was written by the same call.
 * Launches: forward 1, backward 4 (5 with dx).
 * Limits: every required pointer non-NULL, every pointer 16-byte aligned, c_in one of 32, 64, 128 (BALF_ERR_ARG); 1 <= N <= 2^24
 * (BALF_ERR_SHAPE); a workspace smaller than balf_linrelu_train_workspace_bytes gives BALF_ERR_WORKSPACE.  The size query returns
 * 0 outside these limits. */
size_t balf_linrelu_train_workspace_bytes(int N, int c_in);
int balf_linrelu_train_forward(const float *x_dev, const float *w_dev, const float *b_dev, int N, int c_in, float *y_dev,
                               void *stream);
int balf_linrelu_train_backward(const float *g_dev, const float *y_dev, const float *x_dev, const float *w_dev, int N, int c_in,
                                float *dw_dev, float *db_dev, float *dx_dev, void *workspace_dev, size_t workspace_bytes,
                                void *stream);

/* ---- the 2 x 2 max-pool that ends a Down stage, in training form ------------------------------------------------
 * x_dev [B,H,W,C] float32 NHWC -> out_dev [B,H/2,W/2,C] and which_dev [B,H/2,W/2,C] uint8: the raster position 0..3 of the chosen
 * element in its 2 x 2 window, (0,0), (0,1), (1,0), (1,1).  H x W is the INPUT map.
 *   forward    the rule of torch's CPU max_pool2d: the window is scanned in raster order and a value replaces the current one when
 *              it is greater or is NaN, so the first maximum wins, of +0 / -0 the first, of several NaN the last.  out has the
 *              chosen element's bits.
 *   backward   g_dev [B,H/2,W/2,C] and which_dev -> dx_dev [B,H,W,C]: g at the recorded position and +0.0f at the other three.
 *              EVERY element of dx is written (no memset is needed, none is made); nothing but g and which is read.
 * A thread handles four consecutive channels of an output pixel with 16-byte accesses (which: 4 bytes).  Nothing is summed, no
 * atomics, no workspace.  Stream-ordered, nothing synchronised, allocated or read back, capturable.  Launches: 1 each.
 * Limits: 1 <= B <= 65535, H, W >= 1 (BALF_ERR_ARG); H and W even, C a multiple of 4 in 4..256, B * H * W <= 2^24
 * (BALF_ERR_SHAPE); no NULL pointer, every pointer 16-byte aligned (BALF_ERR_ARG). */
int balf_pool_train_forward(const float *x_dev, int B, int H, int W, int C, float *out_dev, unsigned char *which_dev, void *stream);
int balf_pool_train_backward(const float *g_dev, const unsigned char *which_dev, int B, int H, int W, int C, float *dx_dev,
                             void *stream);

/* ---- the buffer sizes of the training units that take their channel width ------------------------------------
 * *workspace_bytes and *saved_bytes of unit at width C on B images whose map, as the unit receives it, is Hc x Wc.
 *   BALF_UNIT_RCAB  balf_rcab_train_*_c, C = 128 or 256; at 256 what balf_rcab_train_workspace_bytes / _saved_bytes return
 *   BALF_UNIT_GMLP  balf_gmlp_train_*_c, C = 128 or 256; at 256 what balf_gmlp_train_workspace_bytes / _saved_bytes return
 *   BALF_UNIT_POOL  balf_pool_train_*: Hc x Wc is the pool's INPUT map; saved is which, B * Hc/2 * Wc/2 * C bytes; workspace is 0
 * Returns BALF_OK, or the code that the unit's entry points give for these sizes (a C the unit does not take: BALF_ERR_SHAPE);
 * an unknown unit or a NULL output: BALF_ERR_ARG.  The two outputs are written only with BALF_OK. */
#define BALF_UNIT_RCAB 0
#define BALF_UNIT_GMLP 1
#define BALF_UNIT_POOL 2
int balf_train_unit_sizes(int unit, int C, int B, int Hc, int Wc, size_t *workspace_bytes, size_t *saved_bytes);

/* ---- the optimiser step over many tensors in one launch ---------------------------------------------------------
 * balf_adam_step: one step of torch.optim.Adam (amsgrad=False, maximize=False, L2 weight decay) on n float32 tensors.  p, g, m, v
 * and numel are HOST arrays of n entries; the pointers in them are device pointers (parameter, gradient, exp_avg, exp_avg_sq of
 * numel[i] elements).  The library copies them by value into the kernel's argument block (the multi-tensor-apply scheme, 2.8 KB at
 * n = 64): no device table, no upload, no workspace, ONE launch for all n tensors.  Workgroup b finds its tensor from per-tensor
 * first-chunk prefixes in the same block (uniform per workgroup) and handles balf_optim_chunk_elems() elements of it, with 16-byte
 * accesses where all of that tensor's pointers are 16-byte aligned, 4-byte accesses otherwise and for the tail.  Both paths run the
 * same operations in the same order: an element's result bits do not depend on alignment or on how the data is cut into tensors.
 *   g' = fma(wd, p, g) (wd != 0; else g)     m' = fma(1 - b1, g', b1 m)     v' = fma(1 - b2, g' g', b2 v)
 *   p' = p - ((lr / bc1) m') / (sqrt(v') / sqrt(bc2) + eps),   bc1 = 1 - b1^step, bc2 = 1 - b2^step
 * b1, 1 - b1, b2, 1 - b2, wd, eps, lr / bc1 and sqrt(bc2) are computed on the host in double and passed as float; everything per
 * element is float32, every operation written here rounded once (the three FMAs are the only fused ones), division and square
 * root correctly rounded.  NaN and Inf in g reach that element alone.  step: the number of THIS step, 1 for the first.
 * balf_sgd_step: p' = p - lr g.
 * g[i] == NULL or numel[i] == 0 skips tensor i: its p, m and v keep their bits.  A call in which every tensor is skipped launches
 * nothing and returns BALF_OK.  g is only read.  Tensors must not overlap one another.
 * BALF_ERR_ARG: n outside 1..BALF_OPTIM_MAX_TENSORS, a NULL array, a NULL p, m or v entry with numel > 0, a pointer that is not
 * 4-byte aligned, a negative numel, lr, eps or weight_decay negative or not finite, a beta outside [0, 1), step < 1.
 * BALF_ERR_SHAPE: more than 2^31 - 1 chunks in all.  Stream-ordered, nothing synchronised, allocated or read back, capturable. */
#define BALF_OPTIM_MAX_TENSORS 64
int balf_optim_chunk_elems(void);            /* elements one workgroup handles; a constant of the build */
int balf_adam_step(int n, float *const *p, const float *const *g, float *const *m, float *const *v, const int64_t *numel,
                   double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream);
int balf_sgd_step(int n, float *const *p, const float *const *g, const int64_t *numel, double lr, void *stream);

/* ---- measurement aid (not part of the data path) ---------------------------------------------
 * Between balf_profile_begin() and balf_profile_end() every kernel launch of the library is bracketed
 * by a hipEvent pair on its launch stream.  balf_profile_end() waits for those events and returns,
 * per slot (balf_profile_slot_name), the summed device time in ms and the number of launches.
 * Global state, not re-entrant; bench.py uses it for the per-kernel roofline figures. */
int balf_profile_num_slots(void);
const char *balf_profile_slot_name(int slot);
int balf_profile_begin(void);
int balf_profile_end(float *ms_total, int *launches);

#ifdef __cplusplus
}
#endif
#endif /* BALF_HIP_H */
