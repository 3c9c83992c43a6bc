/* dim_hip.h — C ABI of libdim_hip.so, the MI355X (gfx950) implementation of
 * deep-image-matching's per-pair hot path (SuperPoint extraction + LightGlue
 * matching).  Plain pointers and sizes only; no torch / numpy types.
 *
 * Conventions
 *   - every pointer named *_dev / documented "device" is HBM memory of the
 *     current HIP device; `stream` is a hipStream_t passed as void* (NULL = the
 *     default stream).  No entry point synchronises unless it says so.
 *   - return value 0 = success; non-zero = failure, dim_last_error() returns a
 *     thread-local message (the Python plugin turns it into an exception; an
 *     allocation failure message contains "out of memory" so that the caller's
 *     tile fallback keyed on that substring keeps working —
 *     reference matchers/matcher_base.py:251-256).
 *
 * Reference interfaces replaced (paths relative to the reference repo root,
 * src/deep_image_matching/...):
 *   dim_sp_*  <-  thirdparty/SuperGluePretrainedNetwork/models/superpoint.py:101-227
 *                 (SuperPoint.__init__/forward) as driven by
 *                 extractors/superpoint.py:107-132 (SuperPointExtractor._extract)
 *   dim_lg_*  <-  thirdparty/LightGlue/lightglue/lightglue.py:300-610
 *                 (LightGlue.__init__/forward) as driven by
 *                 matchers/lightglue.py:102-125 (LightGlueMatcher._match_pairs)
 */
#ifndef DIM_HIP_H
#define DIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIM_HIP_ABI_VERSION 2   /* 2 (round 6): handle structs carry a tune header, dim_tune_set keys 16 - 18, keypoint slots up to 32768, dim_lg_stage_features, the dim_op_* sort entries */

const char* dim_last_error(void);
int dim_abi_version(void);
int dim_device_synchronize(void);
/* Process-wide defaults of the choices a user may make (read at the entry of every later dim_* call; set them before the work starts —
 * they are plain ints, not synchronised against calls running on other threads):
 *   key 1  matrix arithmetic: 2 (default) "fp16x3" = fp32-accurate products on the fp16 matrix cores (2-way splits of the power-of-two-scaled
 *          operands x 3 terms; activations exact up to |x| = 4094 and GUARDED beyond, dim_saturation_read), 1 = "bf16x6" (exact 3-way bf16
 *          splits x 6 terms, no range limit), 0 = plain fp32 MFMA;
 *   fusion on / off (every setting gives the same results to fp32 rounding; the defaults are the fast ones):
 *   key 3  1 (default) SuperPoint conv1a evaluated inside conv1b, 0 = separate kernels;
 *   key 4  1 (default) LightGlue out_proj folded into ffn.0 (split modes), 0 = separate GEMMs;
 *   key 5  1 (default) SuperPoint conv-to-conv activations stored pre-split (fp16x3), 0 = fp32;
 *   key 8  1 (default) LightGlue's K | V attention tile images written by the projection GEMM, 0 = separate pre-split pass;
 *   key 9  1 (default) ALIKED BatchNorm + SELU applied while the consumer stages its input, 0 = separate pass;
 *   key 16 1 (default) SuperPoint's detector tail (convPb 256 -> 65, softmax, depth-to-space) as one kernel in fp16x3, 0 = GEMM + softmax kernels
 *          (bit-identical score maps);
 *   key 17 1 (default) adaptive-depth LightGlue (depth_confidence > 0) evaluates the assignment once, after the layer loop, for every pair with the
 *          weights of the layer it stopped at; 0 = gated assignment launches after every layer (same results);
 *   key 18 1 (default) dim_lg_match with adaptive depth on a handle created for at most two pairs (the per-call plugin hooks) reads the stop
 *          flags back two layers behind the device (an event wait per layer) and does not enqueue the layers that no pair needs; 0 = the call
 *          never touches the host, as calls on larger handles always do (same results);
 *   key 11 LightGlue's feed-forward: 3 (default) ffn.0 + LayerNorm + GELU + ffn.3 + residual as one kernel when the launch fills the GPU,
 *          4 = always, 1 / 2 = LayerNorm + GELU in ffn.0's epilogue only (when large / always), 0 = separate kernels;
 *   kernel-shape selection (same results; the defaults pick by problem size, the other values force a shape — used by the tests to reach
 *   the large-batch kernels with small inputs):
 *   key 0  fp32 conv3x3 kernel variant; key 2  split-precision conv variant (bits 0-1 prefetch variant of the bf16x6 kernels, bit 4 (default
 *          set) 16-row tiles with LDS-DMA weight staging); key 6  split-precision GEMM block (1 default: 128 x 256 when the launch fills the
 *          GPU, 0 = always 128 x 128, 2 = always 128 x 256); key 7  simple_nms tiles (1 default: 64 x 64 on large maps, 0 = 32 x 32,
 *          2 = always 64 x 64); key 10  ALIKED fp16x3 convolution tile rows (16 default, 8, 17 = 16 with streamed weights).
 *   key 20 SuperPoint's descriptor head: 1 (default) convDa / convDb run only on the cells that the keypoints sample when at most 0.8 of the map's
 *          cells can be needed (min(4 capacity, h w) <= 0.8 h w, max_keypoints > 0, fp16x3 with pre-split activations), 0 = always on the whole
 *          map, 2 = on the sampled cells whenever the arithmetic allows (the tests; bit-identical descriptors either way).  (19 is not a key.)
 * Keys 12-15 do not exist in this library: they select research prototypes and timing probes that are compiled only into
 * libdim_hip_research.so (build.build_variant("research", ["-DDIM_RESEARCH"]); csrc/dim_kernels.h) and return an error here.
 * dim_handle_tune_set(handle, key, value) overrides a key for ONE extractor / matcher handle (value < 0: back to the process default). */
int dim_tune_set(int key, int value);
int dim_handle_tune_set(void* handle, int key, int value);

/* Per-launch-site timing with HIP events recorded on the launch stream (bench.py's
 * roofline figure).  dim_profile_start(mask) arms the sites whose bits (1 << DIM_PROF_*) are set;
 * dim_profile_stop() waits for the recorded events and returns the summed kernel time and the
 * number of launches. */
enum {
  DIM_PROF_SP_CONV1A = 0, DIM_PROF_SP_CONV1B, DIM_PROF_SP_CONV2A, DIM_PROF_SP_CONV2B, DIM_PROF_SP_CONV3A,
  DIM_PROF_SP_CONV3B, DIM_PROF_SP_CONV4A, DIM_PROF_SP_CONV4B, DIM_PROF_SP_CONVPA, DIM_PROF_SP_CONVPB,
  DIM_PROF_SP_CONVDA, DIM_PROF_SP_CONVDB, DIM_PROF_SP_POST, DIM_PROF_LG_SELF_ATTN, DIM_PROF_LG_CROSS_ATTN,
  DIM_PROF_LG_GEMMS, DIM_PROF_LG_ASSIGN,
  DIM_PROF_AL_CONV_FULL,  /* ALIKED's full-resolution 3x3 convolutions (block1.conv1 3 -> 16, block1.conv2 16 -> 16): HBM-bound */
  /* dim_ripe_extract in seven spans: statistics + encoder, the decoder's scales 8 / 4 / 2 / 1 (DEC8 + d; each with the resizes that follow it),
   * detection (maxima, map maximum, selection), descriptors (sampling, 960 -> 256, normalisation) */
  DIM_PROF_RIPE_ENCODER, DIM_PROF_RIPE_DEC8, DIM_PROF_RIPE_DEC4, DIM_PROF_RIPE_DEC2, DIM_PROF_RIPE_DEC1, DIM_PROF_RIPE_DETECT, DIM_PROF_RIPE_DESC
};
int dim_profile_start(unsigned long long site_mask);
int dim_profile_stop(double* total_ms, int* launches);

/* fp16x3 range guard.  The default arithmetic represents every activation as two fp16 pieces of 16*x, exact for
 * |x| <= 4094 and saturating beyond.  Every kernel that produces a value a later split consumes checks max|x| of
 * what it writes and bumps a sticky device counter per launch site when the range is exceeded (the results of that
 * call are then NOT fp32-accurate).  dim_saturation_read synchronises `stream`, copies the DIM_SAT_SITES counters to
 * counts_host (may be NULL), returns their sum in *total and zeroes them when reset != 0.  The Python plugins call it
 * after every extract / match and re-run the call in bf16x6 (no range limit) when the sum is non-zero. */
enum {
  DIM_SAT_SP_IMAGE = 0,   /* |image| > 1 or conv1a's weight bound exceeds the range (fused conv1a+conv1b input) */
  DIM_SAT_SP_ENCODER,     /* outputs of conv1b .. conv4b */
  DIM_SAT_SP_HEADS,       /* outputs of convPa / convDa (inputs of the 1x1 head GEMMs) */
  DIM_SAT_LG_INPUT,       /* descriptors handed to dim_lg_match / input_proj output */
  DIM_SAT_LG_QKV,         /* Wqkv / to_qk|to_v outputs incl. the rotated q, k */
  DIM_SAT_LG_FFN,         /* ffn.0 output after LayerNorm+GELU */
  DIM_SAT_LG_DESC,        /* residual stream after ffn.3 */
  DIM_SAT_OP,             /* operator-level entry points (dim_op_*_x6) */
  DIM_SAT_ALIKED,         /* ALIKED: inputs of the split-precision convolutions / GEMMs (image, BatchNorm+SELU outputs, SDDH samples) */
  DIM_SAT_ALIKE,          /* ALIKE: activations stored by the encoder / aggregation convolutions, rows and outputs of the head products */
  DIM_SAT_XFEAT,          /* XFeat: the normalised image, block2's input, the pyramid sum and the activations stored by the trunk convolutions */
  DIM_SAT_NETVLAD,        /* NetVLAD: a NaN pixel, and the activations stored by the thirteen VGG16 convolutions */
  DIM_SAT_RIPE,           /* RIPE: a non-finite pixel, and the activations stored by the encoder and decoder convolutions */
  DIM_SAT_SITES = 16
};
int dim_saturation_read(unsigned* counts_host, unsigned long long* total, int reset, void* stream);
/* Zeroes the counters without reading them: one memset enqueued on `stream`, no synchronisation (what a guarded call does before it starts, to drop
 * anything an earlier unguarded call left behind). */
int dim_saturation_reset(void* stream);

/* Shader-clock probe: writes {s_memtime (shader cycles), s_memrealtime (100 MHz)} to out_dev[2] on `stream`;
 * two probes around a region give its average shader clock = d(cycles) / d(realtime) * 100 MHz (bench.py). */
int dim_op_read_clocks(unsigned long long* out_dev, void* stream);

/* ------------------------------------------------------------------------ */
/* SuperPoint (reference SPN:101-227)                                       */
/* ------------------------------------------------------------------------ */

/* Weights in the reference's own state_dict layout (SPN:128-143): conv weights
 * OIHW fp32, host pointers; they are re-laid out for the kernels at create. */
typedef struct dim_sp_weights {
  const float* conv_w[12]; /* conv1a,1b,2a,2b,3a,3b,4a,4b,convPa,convPb,convDa,convDb */
  const float* conv_b[12];
} dim_sp_weights;

/* Mirrors SuperPoint.default_config (SPN:112-118) + DIM's fix_sampling switch
 * (extractors/superpoint.py:16-27,56-57). */
typedef struct dim_sp_config {
  int nms_radius;           /* >= 0 */
  float keypoint_threshold; /* s > thr */
  int max_keypoints;        /* -1 = keep all (bounded by capacity); top-k up to 32768 (config/superpoint+superglue.yaml: 8000) */
  int remove_borders;
  int fix_sampling;         /* 0: SPN:81-98 sampler, 1: extractors/superpoint.py:16-27 */
} dim_sp_config;

typedef struct dim_sp dim_sp;

/* Builds a resident extractor for images up to max_h x max_w, max_batch images
 * per call, at most capacity keypoints per image (capacity >= max_keypoints
 * when that is >= 0). */
int dim_sp_create(const dim_sp_weights* w, const dim_sp_config* cfg, int max_batch, int max_h, int max_w,
                  int capacity, dim_sp** out);
void dim_sp_destroy(dim_sp* h);

/* images_dev: [batch][H][W] fp32, values already divided by 255
 *             (extractors/superpoint.py:134-146 _frame2tensor).
 * Outputs (device, caller allocated, slot b at offset b*capacity):
 *   kpts_xy_dev  [batch][capacity][2] fp32  (x, y) pixel coordinates (SPN:210)
 *   scores_dev   [batch][capacity]    fp32
 *   desc_dev     [batch][capacity][256] fp32, row-major (N, D) — the transpose of
 *                the reference's (D, N); the Python plugin returns the .T view
 *   n_kpts_dev   [batch] int32
 * Order of keypoints: score-descending when more than max_keypoints survive
 * (torch.topk, SPN:74-78), row-major (y, x) otherwise (SPN:183-186). */
int dim_sp_extract(dim_sp* h, const float* images_dev, int batch, int H, int W, float* kpts_xy_dev, float* scores_dev,
                   float* desc_dev, int32_t* n_kpts_dev, void* stream);

/* Debug/parity taps of the last dim_sp_extract call (device pointers owned by
 * the handle; valid until the next call).  Layouts: encoder [batch][h][w][128],
 * logits [batch][h*w][65], score_map / nms_map [batch][8h][8w],
 * dense_desc (un-normalised convDb output) [batch][h][w][256]. */
int dim_sp_debug_buffers(dim_sp* h, const float** encoder, const float** logits, const float** score_map,
                         const float** nms_map, const float** dense_desc, int* h8, int* w8);

/* fp32 NHWC copy [batch][H/2][W/2][64] of conv1b's pooled output (SPN:162-163) of the last dim_sp_extract call on (batch, H, W):
 * A/B of the convolution variants (dim_tune_set keys 2, 3, 5).  Synchronises the device. */
int dim_sp_debug_conv1b(dim_sp* h, int batch, int H, int W, const float** out_f32, int* h2, int* w2);

/* How the last dim_sp_extract ran the descriptor head.  *slots = 0: on the whole map (*n_rows_dev = NULL).  Otherwise on listed cells: *slots rows
 * were reserved per image and n_rows_dev [batch] (device int32 owned by the handle) holds the number of distinct cells the keypoints sample. */
int dim_sp_desc_rows(dim_sp* h, const int32_t** n_rows_dev, int* slots);

/* Number of NMS survivors above threshold/border per image of the last call
 * (before top-k), device int32 [batch] owned by the handle. */
int dim_sp_candidate_counts(dim_sp* h, const int32_t** ncand_dev);

/* The openly licensed SuperPoint (reference thirdparty/SuperPoint_open/superpoint_pytorch.py, driven by extractors/superpoint_open.py): the
 * layer shapes of dim_sp_weights, every block conv -> ReLU -> BatchNorm(eval) with the 2x2 max-pool BEHIND the BatchNorm, the two 1x1 heads
 * conv -> BatchNorm without ReLU.  Per layer (same order as conv_w) the BatchNorm's weight, bias, running_mean and running_var, [cout] fp32 host
 * pointers, and the one eps of all of them (the reference: 1e-3). */
typedef struct dim_spo_weights {
  const float* conv_w[12];
  const float* conv_b[12];
  const float* bn_gamma[12];
  const float* bn_beta[12];
  const float* bn_mean[12];
  const float* bn_var[12];
  double bn_eps;
} dim_spo_weights;

/* As dim_sp_create; returns an ordinary dim_sp handle (extract, destroy, the debug taps, candidate counts and the tune keys are shared).  s = gamma /
 * sqrt(var + eps) and t = beta - mean * s are formed in double; non-finite values and var + eps <= 0 are rejected.  The eight encoder layers apply
 * s * relu(conv + b) + t in the convolution's epilogue (ahead of the pool); the BatchNorms around the two 1x1 heads are folded into the 1x1
 * weights exactly.  cfg->fix_sampling is ignored (the open network has the one sampler, = 1).  Such a handle runs in the fp16x3 / bf16x6 arithmetic with
 * the fused conv1a only: dim_sp_extract returns an error under precision mode 0 or dim_tune_set key 3 = 0. */
int dim_spo_create(const dim_spo_weights* w, const dim_sp_config* cfg, int max_batch, int max_h, int max_w, int capacity, dim_sp** out);

/* ------------------------------------------------------------------------ */
/* ALIKED (reference ALN = thirdparty/LightGlue/lightglue/aliked.py:561-693, driven by
 * extractors/aliked.py:45-64)                                               */
/* ------------------------------------------------------------------------ */

/* Learnable tensors in the reference's state_dict layout (conv weights OIHW, host pointers;
 * SURVEY.md Appendix A).  BatchNorm running statistics are NOT part of the interface: the
 * reference plugin never calls .eval(), so BatchNorm normalises with the statistics of the
 * current image (quirk Q7, ALX:40-43) and this library does the same. */
typedef struct dim_aliked_weights {
  const float *block1_conv1, *block1_conv2;            /* (16,3,3,3), (16,16,3,3) */
  const float *block2_conv1, *block2_conv2, *block2_ds_w, *block2_ds_b;
  const float *block3_off1_w, *block3_off1_b, *block3_reg1, *block3_off2_w, *block3_off2_b, *block3_reg2, *block3_ds_w, *block3_ds_b;
  const float *block4_off1_w, *block4_off1_b, *block4_reg1, *block4_off2_w, *block4_off2_b, *block4_reg2, *block4_ds_w, *block4_ds_b;
  const float *bn_weight[8], *bn_bias[8];             /* block1.bn1, block1.bn2, block2.bn1, ..., block4.bn2 */
  const float *conv1, *conv2, *conv3, *conv4;          /* 1x1 heads (32,c,1,1) */
  const float *score0, *score2, *score4, *score6;      /* score_head.{0,2,4,6}.weight */
  const float *desc_off0_w, *desc_off0_b, *desc_off2_w, *desc_off2_b, *desc_sf, *desc_agg; /* desc_head.* */
} dim_aliked_weights;

/* ALIKED._default_conf (ALN:562-567) + the geometry row of ALIKED.cfgs (ALN:573-579). */
typedef struct dim_aliked_config {
  int c1, c2, c3, c4, dim, K, M;   /* ALN:573-579: aliked-n16 / n16rot 16,32,64,128,128,3,16; aliked-n32 the same with M = 32; aliked-t16 8,16,32,64,64,3,16 (desc_dev rows are dim floats) */
  int max_num_keypoints;           /* n_limit of DKD (ALN:624-626), up to 32768 (config/aliked.yaml: 8000); <= 0 = n_limit_max 20000 (ALN:571), bounded by capacity */
  double detection_threshold;      /* > 0: threshold mode; <= 0: DKD's top-k mode (exactly max_num_keypoints per image, zero-score pixels filling up,
                                      ALN:150-151) or, with max_num_keypoints <= 0 as well, the mean-score threshold (ALN:161-163) */
  int nms_radius;
} dim_aliked_config;

typedef struct dim_aliked dim_aliked;
int dim_aliked_create(const dim_aliked_weights* w, const dim_aliked_config* cfg, int max_batch, int max_h, int max_w,
                      int capacity, dim_aliked** out);
void dim_aliked_destroy(dim_aliked* h);
/* images_dev: [batch][H][W][in_channels] fp32 (HWC, as the numpy image arrives; already /255,
 *             extractors/aliked.py:66-78), in_channels 3 (RGB) or 1 (repeated to RGB, ALN:679-680).
 * Outputs as dim_sp_extract with D = cfg.dim (128; aliked-t16: 64): kpts (x, y) sub-pixel pixel coordinates (ALN:687),
 * scores = DIM's "scores" i.e. the score DISPERSITIES (quirk Q8), desc row-major (N, dim). */
int dim_aliked_extract(dim_aliked* h, const float* images_dev, int batch, int H, int W, int in_channels, float* kpts_xy_dev,
                       float* scores_dev, float* desc_dev, int32_t* n_kpts_dev, void* stream);
/* Parity taps: un-normalised feature map [batch][Hp][Wp][dim] in the padded frame, score map [batch][H][W]. */
int dim_aliked_debug_buffers(dim_aliked* h, const float** x1234, const float** score_map, int* hp, int* wp, int* pad_t, int* pad_l);

/* ------------------------------------------------------------------------ */
/* ALIKE (reference AKN = thirdparty/alike/alnet.py, AKM = thirdparty/alike/alike.py, AKD =
 * thirdparty/alike/soft_detect.py, driven by extractors/alike.py:22-44)     */
/* ------------------------------------------------------------------------ */

/* Learnable tensors and BatchNorm running statistics in the reference's state_dict layout (conv weights OIHW, host pointers).
 * BatchNorm runs in EVAL mode (AKM:90-94 calls .eval() when a checkpoint is loaded — unlike ALIKED's quirk Q7): it is folded into
 * a per-channel scale and bias at create time (eps 1e-5). */
typedef struct dim_alike_weights {
  const float *block1_conv1, *block1_conv2, *block2_conv1, *block2_conv2;   /* (c1,3,3,3), (c1,c1,3,3), (c2,c1,3,3), (c2,c2,3,3) */
  const float *block3_conv1, *block3_conv2, *block4_conv1, *block4_conv2;   /* (c3,c2,3,3), (c3,c3,3,3), (c4,c3,3,3), (c4,c4,3,3) */
  const float *bn_weight[8], *bn_bias[8], *bn_mean[8], *bn_var[8];          /* block1.bn1, block1.bn2, block2.bn1, ..., block4.bn2 */
  const float *block2_ds_w, *block2_ds_b, *block3_ds_w, *block3_ds_b, *block4_ds_w, *block4_ds_b;   /* blockN.downsample (1x1, with bias; AKN:110,118,126) */
  const float *conv1, *conv2, *conv3, *conv4;   /* (dim/4, c, 1, 1), bias-free (AKN:132-135) */
  const float *convhead1;                        /* (dim, dim, 1, 1); NULL for single-head models (AKN:151-152) */
  const float *convhead2;                        /* (dim + 1, dim, 1, 1) (AKN:153): rows [0, dim) = descriptor head, row dim = score */
} dim_alike_weights;

/* One row of AKM:15-56 + the DKD arguments of extractors/alike.py:28-34. */
typedef struct dim_alike_config {
  int c1, c2, c3, c4, dim, single_head;   /* alike-t 8,16,32,64,64,1; alike-s 8,16,48,96,96,1; alike-n 16,32,64,128,128,1; alike-l 32,64,128,128,128,0 */
  int radius;                             /* 2 in every row (soft-argmax window AKD:89; the NMS radius is 2 regardless, AKD:102) */
  int top_k;                              /* > 0: the top_k highest NMS maxima, score-descending, zero-score pixels (the first non-candidates in row-major
                                             order) filling up (AKD:111-113); <= 0: threshold mode */
  double scores_th;                       /* threshold mode: maxima > scores_th; the image's mean score when <= 0 or when nothing passes (AKD:115-122) */
  int n_limit;                            /* threshold mode: row-major order, or the n_limit highest, score-descending, when more survive (AKD:128-133) */
  int desc_stride;                        /* floats per descriptor row: >= dim, <= 128, multiple of 4, 0 = dim; columns [dim, desc_stride) are written as zeros */
} dim_alike_config;

typedef struct dim_alike dim_alike;
/* capacity (<= 32768) must cover top_k (top-k mode) or n_limit (threshold mode); max_batch <= 64; max_h, max_w >= 16. */
int dim_alike_create(const dim_alike_weights* w, const dim_alike_config* cfg, int max_batch, int max_h, int max_w, int capacity, dim_alike** out);
void dim_alike_destroy(dim_alike* h);
/* images_dev: [batch][H][W][3] fp32 RGB, already /255 (AKM:154).  The network runs on the frame zero-padded at the bottom and right to
 * multiples of 32 (AKM:105-113); the maps are cropped back to H x W (AKM:119-121).
 * kpts (x, y): soft-argmax refined pixel coordinates (AKD:139-178, AKM:163); scores: the score map sampled bilinearly there (AKD:180-187);
 * desc: [batch][capacity][desc_stride], the bilinearly sampled, twice L2-normalised descriptors (AKM:125, AKD:55-69); rows at or past n_kpts are not written. */
int dim_alike_extract(dim_alike* h, const float* images_dev, int batch, int H, int W, float* kpts_xy_dev, float* scores_dev, float* desc_dev,
                      int32_t* n_kpts_dev, void* stream);
/* Parity taps of the last call: score map [batch][H][W], border-cleared NMS map [batch][H][W] (AKD:102-108), padded frame sizes. */
int dim_alike_debug_buffers(dim_alike* h, const float** score_map, const float** nms_map, int* hp, int* wp);

/* ------------------------------------------------------------------------ */
/* XFeat, sparse detectAndCompute (reference XFM = thirdparty/accelerated_features/modules/xfeat.py:50-103,
 * XFN = modules/model.py:123-154, XFI = modules/interpolator.py, driven by extractors/xfeat.py) */
/* ------------------------------------------------------------------------ */

/* The tensors of XFeatModel's state dict that detectAndCompute uses (conv weights OIHW, host pointers); fine_matcher.* is not part of it.
 * A BasicLayer is conv (no bias) -> BatchNorm2d(affine=False) in EVAL mode -> ReLU (XFN:12-25): the BatchNorm is folded into the weights and a
 * bias at create time in fp64 (eps 1e-5).  Order of the 23 BasicLayers: block1.0-3, block2.0-1, block3.0-2, block4.0-2, block5.0-3,
 * block_fusion.0-1, heatmap_head.0-1, keypoint_head.0-2 (geometry: XFN:43-92). */
typedef struct dim_xfeat_weights {
  const float *basic_w[23], *basic_mean[23], *basic_var[23];   /* <layer>.layer.0.weight, <layer>.layer.1.running_mean / running_var */
  const float *skip_w, *skip_b;       /* skip1.1: (24,1,1,1), (24) */
  const float *fusion_w, *fusion_b;   /* block_fusion.2: (64,64,1,1), (64) */
  const float *heat_w, *heat_b;       /* heatmap_head.2: (1,64,1,1), (1) */
  const float *kp_w, *kp_b;           /* keypoint_head.3: (65,64,1,1), (65) */
} dim_xfeat_weights;

typedef struct dim_xfeat_config {
  int top_k;                   /* the top_k highest keys, score-descending (XFM:83-87; always sorted, also below top_k) */
  float detection_threshold;   /* NMS threshold on the keypoint heat map (XFM:74), in [0, 1); the reference's extractor always runs the network's 0.05 */
  int desc_stride;             /* floats per descriptor row: >= 64, <= 128, multiple of 4, 0 = 64; columns [64, desc_stride) are written as zeros */
} dim_xfeat_config;

typedef struct dim_xfeat dim_xfeat;
/* top_k <= capacity <= 32768; max_batch <= 64; max_h, max_w >= 32. */
int dim_xfeat_create(const dim_xfeat_weights* w, const dim_xfeat_config* cfg, int max_batch, int max_h, int max_w, int capacity, dim_xfeat** out);
void dim_xfeat_destroy(dim_xfeat* h);
/* images_dev: [batch][H][W][channels] fp32, channels 1 or 3, any scale (the network normalises every image, XFN:135-136); 32 <= H, W <= the handle's
 * maximum.  The frame is resized bilinearly to (H / 32 * 32, W / 32 * 32) (XFM:236-239; the identity for multiples of 32).
 * kpts (x, y): integer pixels of the resized frame times (W / _W, H / _H) (XFM:96); scores: keypoint heat x reliability (XFM:79); desc:
 * [batch][capacity][desc_stride], the bicubically sampled, L2-normalised descriptors (XFM:90-93); rows at or past n_kpts are not written.
 * As in the reference, a maximum in the last row or column of the resized frame and one at pixel (0, 0) never come out. */
int dim_xfeat_extract(dim_xfeat* h, const float* images_dev, int batch, int H, int W, int channels, float* kpts_xy_dev, float* scores_dev, float* desc_dev,
                      int32_t* n_kpts_dev, void* stream);
/* Parity taps of the last call: the normalised image and the keypoint heat map K1h [batch][_H][_W], the reliability map [batch][_H/8][_W/8], the
 * L2-normalised dense descriptors [batch][_H/8][_W/8][64], and the resized frame's size. */
int dim_xfeat_debug_buffers(dim_xfeat* h, const float** norm_image, const float** k1h, const float** h1, const float** m1, int* hr, int* wr);

/* ------------------------------------------------------------------------ */
/* NetVLAD global descriptor (csrc/netvlad_api.hip, netvlad.hip; NV = thirdparty/hloc/extractors/netvlad.py): the front half of the `retrieval` pair */
/* strategy.  VGG16 features[:-2] (13 3x3 convolutions, pools after layers 2, 4, 7, 10, no ReLU after the last, NV:66-68) -> per-location L2 -> NetVLAD */
/* layer with K clusters (NV:18-39) -> optional whitening Linear(512 K -> whiten_out) + L2 (NV:143-144).                                              */
/* ------------------------------------------------------------------------ */

/* Host pointers, each with its element count (checked against the geometry in create).  conv_w OIHW as NV:86 leaves them (cout, cin, 3, 3) with
 * channels 3,64 | 64,64 | 64,128 | 128,128 | 128,256 | 256,256 | 256,256 | 256,512 | 512,512 x 5;  score_w (K, 512) = score_proj.weight squeezed (NV:99);
 * centers (512, K), already negated (NV:95); whiten_w (whiten_out, 512 K), whiten_b (whiten_out) or both NULL with whiten_out 0 (conf "whiten": False);
 * mean: the checkpoint's averageImage[0, 0] (3 values, NV:118).  K: a multiple of 8 up to 64. */
typedef struct dim_netvlad_weights {
  const float* conv_w[13];
  const float* conv_b[13];
  size_t conv_w_elems[13], conv_b_elems[13];
  const float* mean;      size_t mean_elems;
  const float* score_w;   size_t score_w_elems;
  const float* centers;   size_t centers_elems;
  const float* whiten_w;  size_t whiten_w_elems;
  const float* whiten_b;  size_t whiten_b_elems;
  int K, whiten_out;
} dim_netvlad_weights;

typedef struct dim_netvlad dim_netvlad;
/* max_batch <= 64; max_h, max_w >= 16; max_h x max_w below 2^23 pixels. */
int dim_netvlad_create(const dim_netvlad_weights* w, int max_batch, int max_h, int max_w, dim_netvlad** out);
void dim_netvlad_destroy(dim_netvlad* h);
int dim_netvlad_desc_dim(const dim_netvlad* h);   /* whiten_out, or 512 K without whitening */
/* images_dev: [batch][H][W][3] fp32 RGB in 0..1 (NV:125; the kernel applies clamp(255 x, 0, 255) - mean, NV:126-130), 16 <= H, W <= the handle's
 * maximum.  desc_dev: [batch][dim_netvlad_desc_dim] unit-norm rows.  Arithmetic: the convolutions run as fp16x3 (default, range guard DIM_SAT_NETVLAD)
 * or bf16x6 (dim_tune_set key 1 = 1 or 0) splits on the matrix cores; conv1_1, the head and the whitening are fp32 in every mode.  Every sum has a
 * fixed order: an image's descriptor does not depend on the batch around it.  Only enqueues work on `stream`.
 * Images must be finite.  A NaN pixel is read as 0 - mean (the clamp drops it) where the reference returns a NaN descriptor; it bumps DIM_SAT_NETVLAD in
 * the fp16x3 mode ONLY: the other modes, and therefore the range guard's bf16x6 re-run, have no counter and return a finite descriptor. */
int dim_netvlad_extract(dim_netvlad* h, const float* images_dev, int batch, int H, int W, float* desc_dev, void* stream);
/* Parity tap of the last call: the conv5_3 map [batch][mh][mw][512] (fp32, device) the head consumed. */
int dim_netvlad_debug_buffers(dim_netvlad* h, const float** conv5_map, int* batch, int* mh, int* mw);
/* The head alone on a conv5_3 map [batch][n][512] (device): per-location L2, scores, softmax, aggregation, intra-normalisation, flatten (d K + k),
 * global L2 -> vlad_dev [batch][512 K].  score_dk_dev: (512, K) = score_w TRANSPOSED (the checkpoint's own D x K layout); centers_kd_dev: (K, 512) =
 * centers TRANSPOSED.  workspace: dim_op_netvlad_head_workspace_bytes(batch, n, K) bytes of device memory. */
size_t dim_op_netvlad_head_workspace_bytes(int batch, int n, int K);
int dim_op_netvlad_head_f32(const float* map_dev, int batch, int n, int K, const float* score_dk_dev, const float* centers_kd_dev, void* workspace,
                            float* vlad_dev, void* stream);
/* The whitening alone: y = normalize(W v + b), v_dev [batch][in_dim], w_dev [out_dim][in_dim], y_dev [batch][out_dim]; in_dim a multiple of 4096.
 * W is read once per 16 images.  workspace: dim_op_netvlad_whiten_workspace_bytes(batch, in_dim, out_dim) bytes of device memory. */
size_t dim_op_netvlad_whiten_workspace_bytes(int batch, int in_dim, int out_dim);
int dim_op_netvlad_whiten_f32(const float* v_dev, int batch, int in_dim, const float* w_dev, const float* bias_dev, int out_dim, void* workspace,
                              float* y_dev, void* stream);

/* ------------------------------------------------------------------------ */
/* RIPE (thirdparty/RIPE/ripe: model_zoo/vgg_hyper.py, models/ripe.py = RPM, models/backbones/vgg.py = RPV, vgg_utils.py = RPU,                        */
/* backbone_base.py = RPB, models/upsampler/hypercolumn_features.py = RPH) as extractors/ripe.py drives it: InstanceNorm2d(3) -> VGG19-BN features[:39]  */
/* (twelve conv + BN + ReLU, the map in front of each of the four pools kept) -> DeDoDe-style decoder at scales 8, 4, 2, 1 (ConvRefiner: 1x1, BN, ReLU,  */
/* 1x1; eight depthwise 5x5 + BN + ReLU + 1x1 blocks; (x + x0) / 1.4; 1x1) with bilinear resizes between them -> heat map -> 3x3 maximum + threshold +    */
/* top-k -> hypercolumn rows (960) of the keypoints -> Conv1d(960, 256) -> L2.                                                                         */
/* ------------------------------------------------------------------------ */

/* One convolution followed by an eval-mode BatchNorm (eps 1e-5), host pointers: w, b of the convolution, the BatchNorm's weight, bias, running_mean,
 * running_var.  Folded in fp64 at create time. */
typedef struct dim_ripe_convbn { const float *w, *b, *gamma, *beta, *mean, *var; } dim_ripe_convbn;
/* ConvRefiner of one scale (RPU:32-102): block1 = conv0 (hidden, in, 1, 1) + BN, conv3 (hidden, hidden, 1, 1); hidden_blocks[j] = depthwise
 * (hidden, 1, 5, 5) + BN, pointwise (hidden, hidden, 1, 1); out_conv (out, hidden, 1, 1).  (in, hidden, out) = (512, 512, 257), (512, 256, 129),
 * (256, 128, 65), (128, 64, 2) at scales 8, 4, 2, 1. */
typedef struct dim_ripe_refiner {
  dim_ripe_convbn block1_0;
  const float *block1_3_w, *block1_3_b;
  dim_ripe_convbn dw[8];
  const float *pw_w[8], *pw_b[8];
  const float *out_w, *out_b;
} dim_ripe_refiner;
/* enc[i]: the i-th 3x3 convolution (cout, cin, 3, 3) of torchvision's vgg19_bn with its BatchNorm, channels 3,64 | 64,64 | 64,128 | 128,128 | 128,256 |
 * 256,256 x 3 | 256,512 | 512,512 x 3.  dec[0..3]: scales 8, 4, 2, 1.  desc_w (256, 960), desc_b (256): conv_dim_reduction_coarse_desc. */
typedef struct dim_ripe_weights {
  dim_ripe_convbn enc[12];
  dim_ripe_refiner dec[4];
  const float *desc_w, *desc_b;
} dim_ripe_weights;

typedef struct dim_ripe dim_ripe;
/* max_batch <= 64; max_h, max_w >= 16; max_h x max_w below 2^23 pixels; capacity (rows of the output tables per image) in [1, 32768]. */
int dim_ripe_create(const dim_ripe_weights* w, int max_batch, int max_h, int max_w, int capacity, dim_ripe** out);
void dim_ripe_destroy(dim_ripe* h);
/* RIPE.detectAndCompute (RPM:201-260) on images_dev [batch][H][W][3] fp32 RGB in 0..1 (a gray image repeated to three channels, RPB:55-59),
 * 16 <= H, W <= the handle's maximum.  0 < top_k <= capacity, threshold >= 0 (the key map marks "no candidate" with 0).  Per image b, n = counts_dev[b]
 * rows in descending score, ties by ascending pixel index y W + x: kpts_xy_dev [batch][capacity][2] integer pixel positions (x, y), scores_dev
 * [batch][capacity] = heat / max of the whole heat map, desc_dev [batch][capacity][256] unit-norm rows; rows past n are zero (descriptors, scores) or
 * unspecified (keypoints).  counts_dev[b] == 0 is where the reference raises "No keypoints detected": the caller decides.
 * Arithmetic: the eleven 64..512-channel 3x3 convolutions and every 1x1 convolution run as fp16x3 (default, range guard DIM_SAT_RIPE) or bf16x6
 * (dim_tune_set key 1 = 1 or 0) splits on the matrix cores; the first layer, the depthwise convolutions, the resizes, the detection and the sampling are
 * fp32 in every mode.  Every sum has a fixed order: an image's result does not depend on the batch around it.  Only enqueues work on `stream`. */
int dim_ripe_extract(dim_ripe* h, const float* images_dev, int batch, int H, int W, int top_k, float threshold, float* kpts_xy_dev, float* scores_dev,
                     float* desc_dev, int32_t* counts_dev, void* stream);
/* Parity taps of the last call (fp32, device): heat [batch][H][W]; maps[l] [batch][hs[l]][ws[l]][64 << l], l = 0..3 (the encoder maps in front of the pools). */
int dim_ripe_debug_buffers(dim_ripe* h, const float** heat, const float** maps4, int* hs4, int* ws4, int* batch);
/* The new kernels alone (device pointers, fp32):
 *  dim_op_ripe_dw5x5_f32            out = relu(depthwise5x5(in, pad 2) + bias): in / out [batch][H][W][C], w [25 = 5 dy + dx][C] (BatchNorm folded), C % 32 == 0
 *  dim_op_ripe_resize_bilinear_f32  F.interpolate(bilinear, align_corners=False): channels [c_off, c_off + C) of in [batch][h][w][ld] -> out [batch][H][W][C]
 *  dim_op_ripe_nms3_f32             key [batch][H][W] = heat where it equals its 3x3 window maximum and exceeds threshold (>= 0), else 0
 *  dim_op_ripe_hypercolumn_f32      rows [batch][capacity][960] of the first n_kpts[b] keypoints (x, y) of kpts [batch][capacity][2]: grid_sample
 *                                   (bilinear, align_corners=True, zero padding) of maps4[l] [batch][hs4[l]][ws4[l]][64 << l] at 2 (x, y) / (W - 1, H - 1) - 1 */
int dim_op_ripe_dw5x5_f32(const float* in_dev, const float* w_dev, const float* bias_dev, float* out_dev, int batch, int H, int W, int C, void* stream);
int dim_op_ripe_resize_bilinear_f32(const float* in_dev, int ld, int c_off, int C, int batch, int h, int w, float* out_dev, int H, int W, void* stream);
int dim_op_ripe_nms3_f32(const float* heat_dev, float* key_dev, float threshold, int batch, int H, int W, void* stream);
int dim_op_ripe_hypercolumn_f32(const float* const* maps4, const int* hs4, const int* ws4, const float* kpts_dev, const int32_t* n_kpts_dev, float* rows_dev,
                                int capacity, int batch, int H, int W, void* stream);

/* ------------------------------------------------------------------------ */
/* LightGlue (reference LGN:300-610)                                        */
/* ------------------------------------------------------------------------ */

/* Per-layer tensors in the reference's state_dict layout (nn.Linear weight
 * [out][in], LGN:361-378), host pointers.  d = descriptor_dim, hd = d / heads: 256 and 64 for
 * dim_lg_create (LightGlue), 96 and 96 for dim_lgl_create (LighterGlue). */
typedef struct dim_lg_layer_weights {
  const float *self_Wqkv_w, *self_Wqkv_b;   /* transformers.i.self_attn.Wqkv   (3d,d) rows = head*3hd+dim*3+{q,k,v} */
  const float *self_out_w, *self_out_b;     /* transformers.i.self_attn.out_proj (d,d) */
  const float *self_ffn0_w, *self_ffn0_b;   /* ...self_attn.ffn.0 (2d,2d) */
  const float *self_ln_w, *self_ln_b;       /* ...self_attn.ffn.1 LayerNorm(2d) */
  const float *self_ffn3_w, *self_ffn3_b;   /* ...self_attn.ffn.3 (d,2d) */
  const float *cross_qk_w, *cross_qk_b;     /* transformers.i.cross_attn.to_qk (d,d) */
  const float *cross_v_w, *cross_v_b;       /* ...to_v */
  const float *cross_out_w, *cross_out_b;   /* ...to_out */
  const float *cross_ffn0_w, *cross_ffn0_b, *cross_ln_w, *cross_ln_b, *cross_ffn3_w, *cross_ffn3_b;
  const float *assign_match_w, *assign_match_b; /* log_assignment.i.matchability (1,d),(1,) */
  const float *assign_proj_w, *assign_proj_b;   /* log_assignment.i.final_proj (d,d) */
  const float *token_w, *token_b;               /* token_confidence.i.token.0 (1,d),(1,); NULL for the last layer */
} dim_lg_layer_weights;

typedef struct dim_lg_weights {
  int n_layers;                       /* 9 (LighterGlue: 6) */
  int input_dim;                      /* 256 (SuperPoint), 128 (ALIKED/DISK/SIFT) or 64 (XFeat, LighterGlue) */
  const float *input_proj_w, *input_proj_b; /* (d,input_dim),(d,) or NULL when input_dim == d == 256 (LGN:361-364); required by dim_lgl_create */
  const float* posenc_Wr;             /* posenc.Wr.weight (d / heads / 2, 2) = (32,2), LighterGlue (48,2) */
  const float* confidence_thresholds; /* buffer (n_layers,) (LGN:581-584) */
  const dim_lg_layer_weights* layers; /* [n_layers] */
} dim_lg_weights;

/* LightGlue._default_conf (LGN:301-314); doubles because the reference compares fp32
 * tensors against Python floats.  pruning_min_kpts: LGN:318-323,606-610 (-1 = the CPU
 * path this library is parity-checked against). */
typedef struct dim_lg_config {
  double depth_confidence; /* early stop, disable with -1 */
  double width_confidence; /* point pruning, disable with -1 */
  double filter_threshold;
  int pruning_min_kpts;
} dim_lg_config;

typedef struct dim_lg dim_lg;

int dim_lg_create(const dim_lg_weights* w, const dim_lg_config* cfg, int max_pairs, int max_kpts, dim_lg** out);
/* LighterGlue: LightGlue at another shape (reference thirdparty/accelerated_features/modules/lighterglue.py:12-27: input_dim 64, descriptor_dim
 * 96, ONE head of 96, 6 layers).  Accepts (descriptor_dim, num_heads) = (96, 1); (256, 4) is dim_lg_create; everything else fails with a
 * dim_last_error text.  The result is an ordinary dim_lg: dim_lg_match / destroy / max_kpts / debug_desc (rows of descriptor_dim floats) and
 * dim_handle_tune_set work on it unchanged.  A 96-wide handle runs in the split arithmetics only (dim_tune_set key 1 = 2 or 1, not 0). */
int dim_lgl_create(const dim_lg_weights* w, const dim_lg_config* cfg, int descriptor_dim, int num_heads, int max_pairs, int max_kpts, dim_lg** out);
void dim_lg_destroy(dim_lg* h);
/* Row stride (>= max_kpts, multiple of 4) of the per-point output arrays below. */
int dim_lg_max_kpts(dim_lg* h);

/* The conversion half of featuresDict2Lightglue (matchers/lightglue.py:18-64: descriptors (D, N) -> (N, D), :38-43, and
 * torch.as_tensor(v, dtype=torch.float32, device=device), :62) on the device, for ONE pair whose arrays were uploaded exactly as
 * features.h5 holds them (save_features_h5 with as_half, extractors/extractor_base.py:56-99: float16; SuperPoint / ALIKED write their
 * descriptors as (D, N), extractors/superpoint.py:121-127): fills rows [0, n) of slots 0 and 1 of a feature table
 * kpts_tab_dev [2][cap][2], desc_tab_dev [2][cap][D] (fp32, the layout dim_lg_match reads) and zeroes rows [n, cap).  fp16 -> fp32 is exact,
 * so the table equals what the host conversion produced.  Keypoints 4-byte, descriptors 16-byte aligned; D a multiple of 32. */
typedef struct dim_lg_raw_features {
  const void* kpts_dev;   /* (N, 2) row-major, float32 or float16 */
  const void* desc_dev;   /* (N, D) or (D, N) row-major, float32 or float16 */
  int n;                  /* keypoints (<= cap) */
  int kpts_f16, desc_f16; /* 1: float16, 0: float32 */
  int desc_is_dn;         /* 1: (D, N), 0: (N, D) */
} dim_lg_raw_features;
int dim_lg_stage_features(const dim_lg_raw_features* img0, const dim_lg_raw_features* img1, int cap, int D, float* kpts_tab_dev, float* desc_tab_dev,
                          void* stream);

/* Matches n_pairs pairs in one call.  Features come from a device feature table
 * (slot i = image i, as written by dim_sp_extract):
 *   kpts_tab_dev [n_img][cap][2], desc_tab_dev [n_img][cap][input_dim] (row-major (N,D):
 *   what featuresDict2Lightglue produces, matchers/lightglue.py:38-43), n_tab_dev [n_img],
 *   size_tab_dev [n_img][2] = image_size exactly as DIM feeds it ((H, W)).
 * pair_idx_dev [n_pairs][2] int32 = image slots of (image0, image1); NULL = pair p is
 * slots (2p, 2p+1).  Keypoint counts above the handle's max_kpts are truncated.
 * Outputs (device, caller allocated; NK = dim_lg_max_kpts(h)):
 *   matches_dev   [n_pairs][NK][2] int64 — compact (idx0, idx1) list, idx0 ascending (LGN:543-553)
 *   mscores_dev   [n_pairs][NK]
 *   n_matches_dev [n_pairs]
 *   matches01_dev [n_pairs][2][NK] int32 — matches0 / matches1 (-1 = unmatched)
 *   mscores01_dev [n_pairs][2][NK]       — matching_scores0 / matching_scores1
 *   stop_dev      [n_pairs]              — "stop" (LGN:570)
 *   prune01_dev   [n_pairs][2][NK] int32 — prune0 / prune1
 *   dense_scores_dev: NULL, or [n_pairs][NK+1][NK+1] receiving the inner MxN block of the
 *   log assignment matrix (parity tests only).
 * The call only enqueues work on `stream` and never reads results back — with one exception: on a handle created for at most two pairs, with
 * depth_confidence > 0 (adaptive depth), it waits (spinning on mapped page-locked memory, two layers behind the device) for the pairs' stop flags and
 * stops enqueueing layers once every pair has stopped (dim_tune_set key 18 = 0 turns that off; results are identical either way).  A handle must not be
 * used from two threads at once. */
int dim_lg_match(dim_lg* h, const float* kpts_tab_dev, const float* desc_tab_dev, const int32_t* n_tab_dev,
                 const float* size_tab_dev, int cap, const int32_t* pair_idx_dev, int n_pairs, int64_t* matches_dev,
                 float* mscores_dev, int32_t* n_matches_dev, int32_t* matches01_dev, float* mscores01_dev,
                 int32_t* stop_dev, int32_t* prune01_dev, float* dense_scores_dev, void* stream);

/* Parity taps: final descriptors [2*max_pairs][NK][256], live counts and index maps. */
int dim_lg_debug_desc(dim_lg* h, const float** desc, const int32_t** n_cur, const int32_t** ind);

/* ------------------------------------------------------------------------ */
/* Resident SuperGlue matcher (reference thirdparty/SuperGluePretrainedNetwork/
 * models/superglue.py, SGN; csrc/sg_api.hip, sg_kernels.hip)                */
/* ------------------------------------------------------------------------ */
/* Weights as the HOST prepares them (weights.prepare_superglue_weights, fp64): BatchNorm1d (eval, eps 1e-5) folded into the convolution in
 * front of it, and the attention channels permuted from the module's c = d * 4 + h (view(b, 64, 4, n), SGN:112) to head-major c = h * 64 + d:
 * the ROWS of the three projections and the COLUMNS of merge.  Conv1d(kernel 1) weights are (out, in) row-major, fp32, finite. */
typedef struct dim_sg_layer_weights {
  const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b; /* attn.proj.{0,1,2}: (256,256),(256,) rows head-major */
  const float *merge_w, *merge_b;                 /* attn.merge: (256,256) columns head-major */
  const float *mlp0_w, *mlp0_b;                   /* mlp.0 with mlp.1 (BatchNorm) folded: (512,512) over [x | message] */
  const float *mlp3_w, *mlp3_b;                   /* mlp.3: (256,512) */
} dim_sg_layer_weights;
typedef struct dim_sg_weights {
  const float* kenc_w[5];  /* kenc.encoder.{0,3,6,9,12}, BatchNorm folded into the first four: (32,3),(64,32),(128,64),(256,128),(256,256) */
  const float* kenc_b[5];
  const float *final_proj_w, *final_proj_b; /* (256,256),(256,) */
  float bin_score;
  const dim_sg_layer_weights* layers;       /* [n_layers]: self, cross, self, ... (SGN:216) */
} dim_sg_weights;
typedef struct dim_sg_config {
  int n_layers;        /* len(GNN_layers), read from the state dict: a positive multiple of 2 */
  int descriptor_dim;  /* 256 */
} dim_sg_config;
typedef struct dim_sg dim_sg;

/* Device memory of a handle, N = max_kpts rounded up to 4, P = max_pairs: the score block P * N * N floats (N = 8192, P = 1: 256 MiB;
 * N = 2048, P = 16: 256 MiB), the graph network's activations 2 P N * 2304 floats and the K | V tile images 2 P N * 3072 bytes
 * (N = 8192, P = 1: 144 + 48 MiB).  The (N+1) x (N+1) coupling matrix of the reference is never built. */
int dim_sg_create(const dim_sg_weights* w, const dim_sg_config* cfg, int max_pairs, int max_kpts, dim_sg** out);
void dim_sg_destroy(dim_sg* h);
int dim_sg_max_kpts(dim_sg* h);
/* Matches n_pairs pairs in one call.  The feature table is dim_lg_match's (kpts_tab_dev [n_img][cap][2], desc_tab_dev [n_img][cap][256],
 * n_tab_dev, pair_idx_dev) plus score_tab_dev [n_img][cap], the detection scores the keypoint encoder reads.  size_tab_dev [n_img][2] holds
 * (width, height).  sinkhorn_iterations (>= 0) and match_threshold are per call.  Outputs as dim_lg_match (NK = dim_sg_max_kpts(h)):
 * matches_dev [n_pairs][NK][2] int64 (idx0 ascending), mscores_dev [n_pairs][NK], n_matches_dev [n_pairs], matches01_dev [n_pairs][2][NK]
 * int32 (-1 = unmatched), mscores01_dev [n_pairs][2][NK].  A pair with an empty side gives -1 / 0 everywhere (SGN:255-262).  Runs in the
 * split arithmetics (dim_tune_set key 1 = 2 or 1) under the fp16x3 range guard; only enqueues work on `stream`. */
int dim_sg_match(dim_sg* h, const float* kpts_tab_dev, const float* desc_tab_dev, const float* score_tab_dev, const int32_t* n_tab_dev,
                 const float* size_tab_dev, int cap, const int32_t* pair_idx_dev, int n_pairs, int sinkhorn_iterations, float match_threshold,
                 int64_t* matches_dev, float* mscores_dev, int32_t* n_matches_dev, int32_t* matches01_dev, float* mscores01_dev, void* stream);
/* DEBUG ONLY — dim_sg_debug, dim_sg_debug_layers, dim_sg_sinkhorn, dim_sg_select exist for the parity tests and the stage benchmark; they are not
 * part of the stable ABI and may change or go without a DIM_HIP_ABI_VERSION bump.  A handle with dim_sg_debug_layers set is not a matcher.
 * Parity taps and operator-level tests: the handle's buffers — descriptors [2 P][NK][256] (after the last layer), the score block
 * [P][NK][NK], u and v [P][NK + 1] (pair of m x n: u[m], v[n] = the dustbin entries), the live counts [2 P] and the per-pair skip flags [P]
 * (0 = run, non-zero = empty pair).  dim_sg_sinkhorn / dim_sg_select run the two stages behind the score product on whatever these buffers
 * hold (rows per image <= cap, as in dim_sg_match): what dim_sg_match itself calls. */
int dim_sg_debug(dim_sg* h, float** desc, float** scores, float** u, float** v, int32_t** n_cur, int32_t** done);
/* Parity taps: later dim_sg_match calls stop the graph network after n_layers layers (0: the descriptors tap holds the keypoint encoder's
 * output; < 0: all layers, the default). */
int dim_sg_debug_layers(dim_sg* h, int n_layers);
int dim_sg_sinkhorn(dim_sg* h, int n_pairs, int cap, int sinkhorn_iterations, void* stream);
int dim_sg_select(dim_sg* h, int n_pairs, int cap, float match_threshold, int64_t* matches_dev, float* mscores_dev, int32_t* n_matches_dev,
                  int32_t* matches01_dev, float* mscores01_dev, void* stream);

/* ------------------------------------------------------------------------ */
/* Nearest-neighbour descriptor matching (reference matchers/kornia_matcher.py:
 * kornia.feature.DescriptorMatcher(match_mode, th); csrc/nn_match.hip)      */
/* ------------------------------------------------------------------------ */

/* dm = cdist(desc0, desc1) (Euclidean, from d^2 = max(|a|^2 + |b|^2 - 2 a.b, 0) with the product in the active matrix arithmetic).
 *   nn    every row i -> (i, argmin_j dm[i]), dist = dm
 *   mnn   (i, j) with j = argmin dm[i, :] and i = argmin dm[:, j], dist = dm
 *   snn   rows with d_best / d_second <= th (needs N >= 2), dist = the ratio
 *   smnn  snn(0 -> 1) intersected with the flipped snn(1 -> 0) (needs M, N >= 2), dist = the larger ratio
 * Ties on equal distances go to the lowest index; a 0 / 0 ratio is no match; too few descriptors give an empty list.  The list is always
 * idx0-ascending (kornia's mnn lists by idx1 when M > N: same set). */
enum { DIM_NN_MODE_NN = 0, DIM_NN_MODE_MNN, DIM_NN_MODE_SNN, DIM_NN_MODE_SMNN };
typedef struct dim_nn_config {
  int mode;    /* DIM_NN_MODE_* */
  double th;   /* ratio threshold of snn / smnn (compared in fp32) */
} dim_nn_config;
typedef struct dim_nn dim_nn;
/* dim: descriptor dimension, a multiple of 64 (64, 128, 256). */
int dim_nn_create(const dim_nn_config* cfg, int max_pairs, int max_kpts, int dim, dim_nn** out);
void dim_nn_destroy(dim_nn* h);
/* Row stride (>= max_kpts, multiple of 4) of the per-pair output arrays below. */
int dim_nn_max_kpts(dim_nn* h);
/* Device bytes the handle owns: squared norms, per-tile partial (min, argmin, second) triples, final triples — O(max_kpts^2 / 128) per
 * pair; the max_kpts x max_kpts distance matrix is never stored. */
size_t dim_nn_workspace_bytes(dim_nn* h);
/* Matches n_pairs pairs of a device feature table desc_tab_dev [n_img][cap][dim] fp32 (row-major (N, D)), n_tab_dev [n_img]; pair_idx_dev
 * [n_pairs][2] int32 = image slots of (image0, image1), NULL = pair p is slots (2p, 2p+1).  Counts above the handle's max_kpts are truncated.
 * desc_is_f16_exact != 0: the caller states that every table value is exactly representable in float16 (what features.h5 stores) — under
 * fp16x3 one MFMA term runs instead of three, with bit-identical results on such tables.
 * Outputs (device, caller allocated; NK = dim_nn_max_kpts(h)), the layout of dim_lg_match:
 *   matches_dev [n_pairs][NK][2] int64 compact (idx0, idx1) list, idx0 ascending;  dists_dev [n_pairs][NK];  n_matches_dev [n_pairs].
 * row_stats_dev / col_stats_dev: NULL, or parity taps [n_pairs][3][NK] (4-byte elements): plane 0 = argmin index (int32), plane 1 = min d^2,
 * plane 2 = second-smallest d^2 (fp32), per descriptor of image0 over image1 / of image1 over image0.
 * Inputs with |x| > 4094 under fp16x3 bump the DIM_SAT_OP counter (dim_saturation_read).  The call only enqueues work on `stream`. */
int dim_nn_match(dim_nn* h, const float* desc_tab_dev, const int32_t* n_tab_dev, int cap, int desc_is_f16_exact, const int32_t* pair_idx_dev,
                 int n_pairs, int64_t* matches_dev, float* dists_dev, int32_t* n_matches_dev, float* row_stats_dev, float* col_stats_dev,
                 void* stream);

/* ------------------------------------------------------------------------ */
/* operator-level entry points (each is one kernel launch; used by the      */
/* parity tests and available to integrators)                               */
/* ------------------------------------------------------------------------ */

/* C[M][N] = act(A[M][K] * B + bias) (+ residual); B is [K][N] (ldb) or, when
 * b_is_nk != 0, [N][K] (ldb).  K % 32 == 0, leading dims % 4 == 0. */
int dim_op_gemm_f32(const float* A, int lda, const float* B, int ldb, int b_is_nk, const float* bias,
                    const float* residual, int ldr, float* C, int ldc, int M, int N, int K, int relu, void* stream);

/* fp32-accurate GEMM on the 16-bit matrix cores (csrc/gemm_x6.hip).  dim_x3_create pre-splits a host [K][N] fp32
 * operand for the split mode that is active at the call (dim_tune_set key 1: fp16x3 or bf16x6) and returns an OPAQUE
 * handle (host struct owning the device planes [planes][n_pad][K]); dim_op_gemm_x6_f32 computes
 * C = act(A*W + bias) (+ residual), act 0 none / 1 ReLU / 2 SELU, in the handle's mode.  K % 32 == 0. */
int dim_x3_create(const float* w_kn_host, int K, int N, void** out_handle, int* n_pad_out);
void dim_x3_destroy(void* handle);
int dim_op_gemm_x6_f32(const float* A, int lda, const void* w_x3_handle, int n_pad, const float* bias, const float* residual, int ldr,
                       float* C, int ldc, int M, int N, int K, int act, void* stream);

/* LightGlue's ffn.0 -> LayerNorm(512, eps 1e-5) -> erf-GELU (LGN:141-142,157-158) as ONE kernel: C[M][512] =
 * gelu(layer_norm(A[M][K] * W + bias)); w_x3_handle from dim_x3_create(K, 512) under the default arithmetic. */
int dim_op_gemm_x6_ln_gelu_f32(const float* A, int lda, const void* w_x3_handle, const float* bias, const float* ln_gamma, const float* ln_beta,
                               float* C, int ldc, int M, int K, void* stream);

/* C[M][N] = A[M][K] * B[N][K]^T with both operands fp32 activations (LightGlue's similarity, LGN:271), on the 16-bit matrix cores in the
 * active split arithmetic (|A|, |B| <= 4094 under fp16x3: the callers' producers are range-guarded).  K % 32 == 0, lda / ldb % 4 == 0. */
int dim_op_gemm_x6_nt_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, void* stream);

/* LightGlue's whole feed-forward (LGN:141-142,159,209) as ONE kernel: C[M][256] = residual + gelu(layer_norm(A[M][K] * W0 + bias0)) *
 * W3 + bias3, the 512-wide hidden tensor kept on the compute unit.  w0 from dim_x3_create(K, 512); w3 from dim_x3_create_kperm(512,
 * 256) (the same split, rows of every 16-step stored in the order the kernel's register-resident operand presents them). */
int dim_x3_create_kperm(const float* w_kn_host, int K, int N, void** out_handle, int* n_pad_out);
int dim_op_ffn_fused_f32(const float* A, int lda, const void* w0_x3_handle, const float* bias0, const float* ln_gamma, const float* ln_beta,
                         const void* w3_x3_kperm_handle, const float* bias3, const float* residual, int ldr, float* C, int ldc, int M, int K,
                         void* stream);

/* The matchers' attention on caller-supplied projections, through the launchers dim_lg_match / dim_sg_match run (csrc/lg_attn.hip, lg_attn_x6.hip,
 * lg_attn_d96.hip; several launches: [rotary |] K | V pre-split, attention [, merge of a split key range]), in the arithmetic of dim_tune_set key 1.
 *   width 256: 4 heads of 64, qkv rows of 768, enc rows cos[32] | sin[32], softmax scale 1/8.  fp16x3, bf16x6 or fp32.
 *   width 96:  1 head of 96, qkv rows of 288, enc rows cos[48] | sin[48], scale 96^-0.5 (cross: 96^-0.25 on either side).  fp16x3 or bf16x6 only.
 *   kind 0  LightGlue self: rows [q | k | v]; every pair (x[2f], x[2f + 1]) of a head of q and k is rotated by (cos[f], sin[f]) of its row (LGN:41-54).
 *           In the fp32 arithmetic the rotation is written back: q and k of qkv come back rotated.
 *   kind 1  LightGlue cross: rows [qk | v | unused]; item i attends to the keys and values of item i ^ 1, no rotation (enc may be NULL).
 *   kind 2 / 3  SuperGlue self / cross (width 256, split arithmetics only): rows [q | k | v] in both, no rotation; 3 reads k, v of item i ^ 1.
 * qkv [n_items][nmax][3 width], enc [n_items][nmax][64 | 96], ctx [n_items][nmax][width]: 16-byte aligned.  n_dev [n_items]: live
 * rows per item, each <= nsel <= nmax (launch shapes follow nsel, strides follow nmax); done_dev [n_items / 2]: a pair with done != 0 is skipped.
 * ctx row r of item i = softmax(q_r K^T scale) V over the first n[key item] keys; an empty key set gives a row of zeros.  Rows at or past n[i] and
 * the rows of skipped pairs are not written, and no row of qkv at or past n[item] is read.
 * split_items: 0 = the key range is never cut.  Otherwise, when n_items <= split_items, the launchers' own rule cuts it into 4, 2 or 1 parts for
 * cdiv(nsel, 128) * heads * n_items below 256, below 512, or above (what the matchers do for small batches), and a merge kernel follows.
 * workspace: dim_op_lg_attention_workspace_bytes(...) bytes, 16-byte aligned; nothing is read from it that this call has not written.
 * fp16x3 range guard: DIM_SAT_OP counts |k| > 4094 after the rotation (width 96: after the rotation and the 96^-0.25 scale, and |v| as well).  At
 * width 256 v is NOT checked here: in the matchers the projection GEMM that produces it reports it; a caller of this entry keeps |v| <= 4094. */
size_t dim_op_lg_attention_workspace_bytes(int width, int n_items, int nmax, int split_items);
int dim_op_lg_attention_f32(int width, int kind, float* qkv, const float* enc, const int32_t* n_dev, const int32_t* done_dev, float* ctx, int n_items,
                            int nmax, int nsel, int split_items, void* workspace, void* stream);
/* The large-batch form of dim_lg_match's attention (width 256, fp16x3, kind 0 | 1): the projection qkv = x W + bias (x [n_items][nmax][256], W from
 * dim_x3_create(256, 768) for kind 0, (256, 512) for kind 1) writes the K | V tile images in its epilogue (rotary included), no pre-split pass runs, and
 * cross attention takes its Q operand from the item's own K image.  qkv receives the fp32 projection (live rows), ctx as above.  An error when the
 * projection GEMM does not fuse the images at this shape (n_items, nsel).  Same workspace; DIM_SAT_OP counts |q|, |k|, |v| > 4094 as well. */
int dim_op_lg_qkv_attention_f32(int kind, const float* x, const void* w_x3_handle, const float* bias, const float* enc, const int32_t* n_dev,
                                const int32_t* done_dev, float* qkv, float* ctx, int n_items, int nmax, int nsel, int split_items, void* workspace,
                                void* stream);

/* What turns the LightGlue / LighterGlue network output into the integers a caller sees (csrc/lg_kernels.hip, the 96-wide forms in lgl_kernels.hip):
 * token confidence and the early-stop decision, point pruning, the double-softmax assignment, mutual-argmax filtering with the scatter back to the
 * un-pruned index space.  Each entry fills the matchers' state over the caller's device tensors and calls the matchers' own launcher; an entry checks
 * the pointers it uses (named with it below) and leaves the others alone, so they may be NULL.  item = 2 * pair + side.  Everything is ragged: rows at
 * or past n_cur[item] are neither read nor written, and a pair is skipped unless its done flag selects it.
 *   width 256 | 96: desc rows of `width` floats, enc rows of 64 | 96 (cos | sin).  Launch shapes follow nsel (n_cur[item] <= nsel <= nmax), strides nmax. */
typedef struct dim_lg_head_state {
  int32_t width, n_pairs, nmax, nsel;
  float* desc;      /* [items][nmax][width] */
  float* enc;       /* [items][nmax][64 | 96] */
  float* sim;       /* [pairs][nmax][nmax]: similarity of row (side 0 point) x column (side 1 point) */
  float* conf;      /* [items][nmax] token confidence */
  float* mtch;      /* [items][nmax] matchability (sigmoid) */
  float* zls;       /* [items][nmax] logsigmoid of the matchability logit */
  float* rmax;      /* [items][nmax] maximum ... */
  float* rlse;      /* [items][nmax] ... and log of the sum of exp(sim - maximum) of a row (side 0) / a column (side 1) */
  float* best;      /* [items][nmax] best log-assignment per row / column */
  int32_t* arg;     /* [items][nmax] its index: the column of a row (side 0), the row of a column (side 1); the first one among equals */
  int32_t* n_cur;   /* [items] live points */
  int32_t* n_new;   /* [items] live points after the pruning pass */
  int32_t* n_orig;  /* [items] points before any pruning */
  int32_t* ind;     /* [items][nmax] original index of each live point */
  int32_t* dest;    /* [items][nmax] where the pruning pass moves a live point (-1: dropped) */
  int32_t* prune;   /* [items][nmax] layers survived, by ORIGINAL index */
  int32_t* done;    /* [pairs] 0 running, > 0 stopped at that layer, < 0 left without keypoints */
  int32_t* cnt_lt;  /* [pairs] points of the pair with confidence < threshold */
} dim_lg_head_state;
/* conf = sigmoid(desc . w_tok + b_tok) (0 when !use_token), mtch = sigmoid(desc . w_match + b_match) per live point of the running pairs (done == 0);
 * cnt_lt[pair] += the number of its points with conf < thr (use_token only).  Uses desc, conf, mtch, cnt_lt, n_cur, done. */
int dim_op_lg_confidence_f32(const dim_lg_head_state* hs, const float* w_tok, const float* b_tok, const float* w_match, const float* b_match, float thr,
                             int use_token, void* stream);
/* Per running pair: last -> done = layer + 1; else early and 1 - cnt_lt / (n_orig[0] + n_orig[1]) > depth_conf -> done = layer + 1.  cnt_lt of every
 * pair returns to 0; a stopped pair keeps its layer.  Uses done, cnt_lt, n_orig. */
int dim_op_lg_decide(const dim_lg_head_state* hs, int layer, float depth_conf, int early, int last, void* stream);
/* Pruning of the running pairs' items with n_cur > pruning_min: a point stays if mtch > 1 - width_conf (compared in fp32) or, with use_token,
 * conf <= thr.  dest and n_new are written; the kept rows of desc, enc and ind move to the front in order; prune[ind] += 1 for every kept point; n_cur =
 * n_new; a side pruned to nothing sets done = -(layer + 2).  When nothing goes on a side, its rows and the workspace are not touched.  Uses desc, enc,
 * conf, mtch, n_cur, n_new, ind, dest, prune, done.  workspace: dim_op_lg_prune_workspace_bytes(...) bytes, 16-byte aligned. */
size_t dim_op_lg_prune_workspace_bytes(int width, int n_items, int nmax);
int dim_op_lg_prune(const dim_lg_head_state* hs, int layer, double width_conf, float thr, int use_token, int pruning_min, void* workspace, void* stream);
/* The log-assignment of LightGlue (LGN:246-275) on a caller-supplied similarity, for the pairs with done == tag (tag > 0; w_match [width], b_match [1])
 * or, tag == 0, every pair with done > 0 (w_match [layers][width], b_match [layers], row done - 1):
 *   score(i, j) = log_softmax(sim, columns)(i, j) + log_softmax(sim, rows)(i, j) + logsigmoid(z0[i]) + logsigmoid(z1[j]),  z = desc . w_match + b_match.
 * Writes zls, rmax, rlse, best, arg (both sides) and, if dense is not NULL, score into dense [pairs][nmax + 1][nmax + 1] (live entries only).
 * Which kernels run follows nmax and nsel as in the matchers: the 16-byte kernels when nmax is a multiple of 4 and nsel <= 4096 (rows held in 8
 * registers per lane up to nsel 2048, 16 above), the generic ones otherwise.  Uses desc, sim, zls, rmax, rlse, best, arg, n_cur, done. */
int dim_op_lg_assign_f32(const dim_lg_head_state* hs, int tag, const float* w_match, const float* b_match, float* dense, void* stream);
/* LightGlue's filter_matches (LGN:281-297) and the scatter through ind (LGN:543-566), one pair per workgroup.  Row i and column j match when
 * arg0[i] == j and arg1[j] == i; the match is valid when exp(best0[i]) > filter_thr.  An arg outside [0, n_cur of the other side) means "no match".
 *   matches [pairs][out_cap][2] (int64), mscores [pairs][out_cap]: the valid matches in row order as ORIGINAL indices, the first out_cap of them;
 *   n_matches [pairs] = min(count, out_cap);  mfull [items][nmax] (-1: none), msfull [items][nmax] (0 unless mutual): by original index, complete;
 *   stop [pairs] = |done|;  prune_out [items][nmax] = prune (prune_enabled) or n_layers below n_orig, 0 above.  A pair with done <= 0 has no matches.
 * Uses best, arg, n_cur, n_orig, ind, prune, done. */
int dim_op_lg_finalize(const dim_lg_head_state* hs, int n_layers, int prune_enabled, float filter_thr, int out_cap, int64_t* matches, float* mscores,
                       int32_t* n_matches, int32_t* mfull, float* msfull, int32_t* stop, int32_t* prune_out, void* stream);

/* 3x3/s1/p1 conv, NHWC fp32, weights [9][cin][cout], bias+ReLU and optional
 * 2x2 max-pool fused (SPN:161-171).  cin in {64,128}, cout % 64 == 0. */
int dim_op_conv3x3_nhwc_f32(const float* in, const float* w_tap_cin_cout, const float* bias, float* out, int batch,
                            int H, int W, int cin, int cout, int pool2x2, int relu, void* stream);

/* simple_nms (SPN:47-63) on [batch][H][W] score maps, radius 0..6; non-maxima -> 0.  Scores must be >= +0 (what the reference feeds it: softmax
 * outputs; ALIKED: sigmoids) — the kernel keeps a per-pixel mark in the sign bit. */
int dim_op_simple_nms_f32(const float* score_map, float* out, int batch, int H, int W, int radius, void* stream);

/* Keypoint selection on [batch][H][W] NMS maps, the chain dim_sp_extract and dim_aliked_extract run after the NMS (csrc/sp_post.hip: count / scan /
 * emit rows, top-k, zero fill; several launches).  Per image:
 *   candidates = the pixels with  v > threshold  and  border <= y < H - border,  border <= x < W - border,  in row-major order; n of them.
 *                threshold_dev (device, one float per image) replaces `threshold` when it is not NULL.
 *   k < 0, or n <= k without sort_always:  the first min(n, capacity) candidates, row-major (SPN:75-76, torch.nonzero order).
 *   otherwise:                             the min(n, k) highest, score descending, equal scores by ascending pixel index (y * W + x).
 *   zero_fill (DKD's top-k mode, ALN:150-151; scalar threshold only, k <= H * W): an image that kept fewer than k is filled up to k with the
 *                FIRST NON-CANDIDATE PIXELS IN ROW-MAJOR ORDER, border pixels included, each with score 0.  (torch.topk takes some zero-score
 *                pixels there too; which ones is an accident of its sort.)
 * DOMAIN: scores and thresholds must be >= +0 (softmax / sigmoid outputs and 0 at suppressed pixels): the sort key is the score's bit pattern,
 * which orders like the value only for non-negative floats.  k != 0, k <= capacity, k <= 32768; H * W * batch < 2^31.
 * Outputs (device): kpts_xy [batch][capacity][2] = (x, y) as floats, scores [batch][capacity], n_out [batch]; rows at or past n_out[b] are not
 * written.  n_candidates [batch] (NULL: not reported) receives n, also when the output was truncated to the capacity.
 * workspace: dim_op_select_topk_workspace_bytes(batch, H, W, k) bytes of device memory, 16-byte aligned; it may be reused by later calls of any
 * shape that fits (nothing is read from it before it is written).  nms must be 16-byte aligned.  The call only enqueues work on `stream`. */
size_t dim_op_select_topk_workspace_bytes(int batch, int H, int W, int k);
int dim_op_select_topk_f32(const float* nms, int batch, int H, int W, float threshold, const float* threshold_dev, int border, int k, int capacity,
                           int sort_always, int zero_fill, void* workspace, float* kpts_xy, float* scores, int32_t* n_out, int32_t* n_candidates,
                           void* stream);

/* XFeat's selection (XFM:74-87) on caller-supplied maps: k1h [batch][H][W] (keypoint heat), h1 [batch][H/8][W/8] (reliability); H, W multiples of 8.
 * candidate = k1h > threshold and no larger value in its 5 x 5 window (ONE pass: equal values are all kept); key = nearest(k1h) * bilinear(h1) through
 * the reference's samplers (XFI), so the last row / column (nearest sample outside the map) and pixel (0, 0) (the padding position) have key 0 and are
 * dropped like every key <= 0.  Then the chain of dim_op_select_topk_f32 on the key map with sort_always: the min(n, top_k) highest keys, descending.
 * Outputs as there (scores = keys).  workspace: dim_op_xfeat_select_workspace_bytes(batch, H, W, top_k) bytes, 16-byte aligned.  top_k <= capacity <= 32768. */
size_t dim_op_xfeat_select_workspace_bytes(int batch, int H, int W, int top_k);
int dim_op_xfeat_select(const float* k1h, const float* h1, int batch, int H, int W, float threshold, int top_k, int capacity, void* workspace, float* kpts_xy,
                        float* scores, int32_t* n_out, void* stream);

/* SuperPoint's descriptor sampling (SPN:81-98,215; fix_sampling != 0: the variant of extractors/superpoint.py:16-27) as one kernel: the dense
 * map dense_nhwc [batch][h][w][256] (NOT normalised: every cell is L2-normalised on the fly, eps 1e-12) is sampled bilinearly (zero padding)
 * at the first n_kpts[b] <= capacity keypoints of kpts_xy [batch][capacity][2] (pixels of the 8h x 8w image) and L2-normalised again:
 * desc [batch][capacity][256]; rows at or past n_kpts[b] are not written.  A keypoint whose cells are all zero gives a zero descriptor. */
int dim_op_sample_descriptors_f32(const float* dense_nhwc, const float* kpts_xy, const int32_t* n_kpts, float* desc, int batch, int h, int w,
                                  int capacity, int fix_sampling, void* stream);

/* The same convolution on the 16-bit matrix cores at fp32 accuracy (csrc/conv_x6.hip): weights are pre-split from
 * the reference's OIHW fp32 layout by dim_convx6_create for the active split mode (opaque handle, free with
 * dim_x3_destroy). */
int dim_convx6_create(const float* w_oihw_host, int cin, int cout, void** out_handle);
int dim_op_conv3x3_x6_nhwc_f32(const float* in, const void* w_x6_handle, const float* bias, float* out, int batch, int H, int W,
                               int cin, int cout, int pool2x2, int relu, void* stream);

/* The implicit-GEMM NHWC convolution of ALIKE's encoder and XFeat's trunk (csrc/nhwc_conv.hip) as one layer:
 *   out[b][y][x][co] = act( sum_{tap,ci} in[b][stride y + dy][stride x + dx][ci] w[co][ci][tap] + sum_ci in2[b][y][x][ci] w2[co][ci] + bias[co] )
 * dim_nhwc_conv_create takes the reference's OIHW fp32 weight (cout <= 128, kernel 3 with zero padding 1 or kernel 1, stride 1 | 2), optionally the
 * 1x1 OIHW weight w2 of a second input with cin2 channels at output resolution (NULL / 0: none), bias [cout] and relu; free with dim_nhwc_conv_destroy.
 * All maps are NHWC fp32 with channel strides padded up to multiples of 16: in [batch][in_h][in_w][pad16(cin)], in2 [batch][H][W][pad16(cin2)], out
 * [batch][H][W][pad16(cout)]; padding channels of the inputs must hold zeros and those of the outputs are written as zeros.  Input positions outside
 * in_h x in_w read as zero.  img3 (cin = 3): in is the [batch][in_h][in_w][3] image, which may be smaller than the H x W frame.  unfold8 (cin = 64,
 * kernel 1): in is the plane [batch][8 H][8 W] read as its 8 x 8 unfolding, channel = 8 dy + dx.  pool = 2 | 4 (H, W multiples of it): the max-pooled
 * copy of the activated map goes to pooled [batch][H/pool][W/pool][pad16(cout)] as well; 0: none.  stride 2, unfold8 and img3 exclude each other, and
 * the first two exclude in2 and pool, img3 excludes in2.  Arithmetic: fp16x3 when dim_tune_set key 1 is 2 (DIM_SAT_OP counts stored |values| > 4094), fp32 MFMA otherwise. */
typedef struct dim_nhwc_conv dim_nhwc_conv;
int dim_nhwc_conv_create(const float* w_oihw, int cout, int cin, int ksize, int stride, const float* w2_oihw, int cin2, const float* bias, int relu,
                         dim_nhwc_conv** out);
void dim_nhwc_conv_destroy(dim_nhwc_conv* h);
int dim_op_nhwc_conv_f32(const dim_nhwc_conv* h, const float* in, int in_h, int in_w, int img3, int unfold8, const float* in2, float* out, float* pooled,
                         int pool, int batch, int H, int W, void* stream);

/* conv1a: [batch][H][W] -> [batch][H][W][64], weights [9][64], bias, ReLU. */
int dim_op_conv1a_f32(const float* in, const float* w_tap_cout, const float* bias, float* out, int batch, int H, int W,
                      void* stream);

/* ---- tile preselection on device (csrc/tile_ops.hip) ------------------------------------------------
 * Replaces the host steps of tile_selection's PRESELECTION branch (matchers/matcher_base.py:1054-1133):
 * cv2.resize(img, size, interpolation=cv2.INTER_AREA) of a single-channel fp32 image (MB:1068-1069; the
 * OpenCV 4.11 decimation table restated; an enlarging size takes OpenCV's bilinear emulation of INTER_AREA),
 * optionally followed by frame2tensor's
 * /255 (MB:1393-1398); and the vote count "matches whose two end points fall into tile t0 of image 0 and
 * tile t1 of image 1" (points_in_rect / get_tile_bounding_box, MB:1124-1133, strict inequalities).
 * matches is dim_lg_match's (S,2) int64 list with its device-side count; keypoints are the down-sampled
 * images' (x,y) and are divided by scale0/scale1 in fp32 as numpy does; origins are (x,y) int32 pairs;
 * votes[T0*T1] is zeroed by the call. */
int dim_op_resize_area_f32(const float* src, int H, int W, float* dst, int h, int w, int div255, void* stream);
/* The tail of _extract_by_tile (extractors/extractor_base.py:330-390) on the device: per-tile tables kpts [n_tiles][cap][2], scores
 * [n_tiles][cap], desc [n_tiles][cap][D], live counts n_tab [n_tiles] (device), tile origins (x, y) int32 and the tile numbers as
 * floats (tile_ids, the values of "tile_idx") -> keypoints shifted to image coordinates, those within 2 px of the (image_h,
 * image_w) border dropped, concatenated in tile order and, with select_unique, sorted + de-duplicated exactly like
 * np.unique(kpts, axis=0, return_index=True) (lexicographic by (x, y), first occurrence kept).  Outputs (device, sized for
 * n_tiles * cap rows): out_kpts [N][2], out_scores [N], out_tile_idx [N], out_desc = the contiguous (D, N) array in the first
 * D * N floats, *n_out = N.  workspace: dim_op_merge_tiles_workspace_bytes(n_tiles, cap) bytes of device memory. */
size_t dim_op_merge_tiles_workspace_bytes(int n_tiles, int cap);
int dim_op_merge_tiles(const float* kpts_tab, const float* scores_tab, const float* desc_tab, const int32_t* n_tab, const int32_t* origins_xy,
                       const float* tile_ids, int n_tiles, int cap, int D, int image_h, int image_w, int select_unique, void* workspace,
                       float* out_kpts, float* out_scores, float* out_tile_idx, float* out_desc, int32_t* n_out, void* stream);
/* Integer bookkeeping of tile-wise matching on the device (csrc/sort_ops.hip) — get_features_by_tile's boolean masks (matchers/matcher_base.py:1380-1391)
 * and _match_by_tile's np.unique(matches, axis=0) (:452-459) without host-language sort / unique calls:
 *  (ld_*: row strides in floats — the three columns may be views of one packed [n][4 + D] table)
 *  dim_op_tile_counts      counts[t] = keypoints of the merged table with tile_idx == t (tile_idx: the float values of "tile_idx");
 *  dim_op_group_by_tile    the merged table (tile_idx [n], kpts [n][2], desc [n][D]) -> per-tile tables: tile t goes to table row row_of_tile[t]
 *                          (-1: not needed), its keypoints in their ORIGINAL order (= the boolean-mask order) into kt [rows][cap][2], dt [rows][cap][D],
 *                          it [rows][cap] int64 (index in the merged table), nt [rows] live counts.  The tables must arrive zeroed.
 *  dim_op_tile_match_keys  dim_lg_match's lists of a batch of tile pairs (matches [n_pairs][nk][2] int64, n_matches) -> keys [n_pairs][nk] =
 *                          slot << 40 | it[row0][m0] << 20 | it[row1][m1] (pair_rows [n_pairs][2] = the two table rows, slot = the image pair), ~0 for dead rows;
 *  dim_op_unique_match_rows  n keys -> per slot the UNIQUE (idx0, idx1) rows in lexicographic order (np.unique(axis=0)): rows [n_slots][cap_m][2]
 *                          (int32, or int64 with rows_are_i64), cnt[slot] = min(rows of the slot, cap_m), n_full[slot] (optional) = before that cut. */
int dim_op_tile_counts(const float* tile_idx_dev, int ld_tile, int n, int n_tiles, int32_t* counts_dev, void* stream);
size_t dim_op_group_by_tile_workspace_bytes(int n, int n_tiles);
int dim_op_group_by_tile(const float* tile_idx_dev, int ld_tile, const float* kpts_dev, int ld_kpts, const float* desc_nd_dev, int ld_desc, int n, int D,
                         const int32_t* row_of_tile_dev, int n_tiles, int cap, float* kt_dev, float* dt_dev, long long* it_dev, int32_t* nt_dev, void* workspace, void* stream);
int dim_op_tile_match_keys(const long long* matches_dev, const int32_t* n_matches_dev, const long long* it_dev, const int32_t* pair_rows_dev, const int32_t* slot_dev,
                           int n_pairs, int nk, int cap, unsigned long long* keys_dev, void* stream);
size_t dim_op_unique_match_rows_workspace_bytes(long long n);
int dim_op_unique_match_rows(const unsigned long long* keys_dev, long long n, int n_slots, int cap_m, int rows_are_i64, void* rows_dev, int32_t* cnt_dev,
                             int32_t* n_full_dev, void* workspace, void* stream);
/* Tile slicing of _extract_by_tile (extractors/extractor_base.py:279-328) on the device: image_dev [H][W][C] fp32 as the numpy array
 * arrived (0..255), origins (x, y) int32 per tile (negative / overhanging = the Tiler's zero padding) ->
 * out_dev [n_tiles][tile_h][tile_w][C], optionally / 255 (_frame2tensor). */
int dim_op_gather_tiles_f32(const float* image_dev, int H, int W, int C, const int32_t* origins_xy_dev, int n_tiles, int tile_h, int tile_w,
                            float* out_dev, int div255, void* stream);
/* cv2.resize(img, size, interpolation=cv2.INTER_LINEAR) (pixel-centre bilinear, OpenCV 4.11 restated): what
 * utils/image.py:52-57 resize_image uses when the target size enlarges the image — quality HIGHEST in
 * extractor_base.py:392-412 and tile_selection (matcher_base.py:1026-1034). */
int dim_op_resize_linear_f32(const float* src, int H, int W, float* dst, int h, int w, int div255, void* stream);
int dim_op_tile_pair_votes(const float* kpts0_xy, const float* kpts1_xy, const long long* matches, const int* n_matches_dev,
                           int max_matches, float scale0, float scale1, const int* origins0_xy, int T0, const int* origins1_xy, int T1,
                           int tile_w, int tile_h, int* votes, void* stream);

/* ---- writers off the critical path (csrc/export_ops.hip) -------------------------------------------------------
 * The device half of save_features_h5 (extractors/extractor_base.py:56-99) for a batch of dim_sp_extract / dim_aliked_extract
 * tables: float32 -> float16 (round-to-nearest-even, overflow -> inf: numpy's astype(float16), EB:60-67), descriptors
 * (N, D) -> (D, N) (extractors/superpoint.py:121-127), un-padding to the live counts.  out_f16_dev receives
 * [batch][slot] fp16 with slot = dim_pack_features_slot_halves(cap, D) = cap * (4 + D) elements:
 *   [0, 2n) keypoints (n,2) | [2cap, 2cap+n) scores | [3cap, 3cap+n) tile_idx (zeros when tile_idx_dev is NULL) |
 *   [4cap, 4cap + D n) descriptors (D, n) with row stride n;  n = min(n_kpts[b], cap).  D % 64 == 0.
 * One device-to-host copy of the slots is then the byte image of the datasets features.h5 stores. */
size_t dim_pack_features_slot_halves(int cap, int D);
int dim_op_pack_features_f16(const float* kpts_dev, const float* scores_dev, const float* desc_dev, const int32_t* n_kpts_dev,
                             const int32_t* tile_idx_dev, int batch, int cap, int D, void* out_f16_dev, void* stream);
/* The accept / reject rules that follow the estimator in MatcherBase.match (matchers/matcher_base.py:287-334) on the device
 * tables of dim_lg_match + dim_gv_fundamental: a pair with fewer than 8 raw matches, fewer than min_inliers inliers or an
 * inlier ratio below min_ratio (fp64 quotient, as Python evaluates it) gets n_verified = -1; otherwise verified_dev
 * [n_pairs][nk][2] receives the inlier rows in order and n_verified their count. */
int dim_op_filter_matches(const int64_t* matches_dev, const int32_t* n_matches_dev, const unsigned char* mask_dev, int nk, int n_pairs,
                          int min_inliers, double min_ratio, int64_t* verified_dev, int32_t* n_verified_dev, void* stream);

/* End-of-job exchange of the per-rank match tables (SURVEY §8(e) phase 4; no reference counterpart — the reference is single
 * process): dim_lg_match's (S,2) int64 lists + scores -> [n_pairs][nk][3] int32 rows (idx0, idx1, score bits), zero beyond
 * n_matches, ready for ONE all-gather of a flat int32 buffer; and back to int64 / fp32 tables, reading row src_of_pair[p]
 * of the gathered buffer for output pair p (NULL = identity), which undoes the round-robin shard order. */
int dim_op_pack_match_rows(const int64_t* matches_dev, const float* scores_dev, const int32_t* n_matches_dev, int nk, int n_pairs,
                           int32_t* rows_dev, void* stream);
int dim_op_unpack_match_rows(const int32_t* rows_dev, const int32_t* src_of_pair_dev, int nk, int n_pairs, int64_t* matches_dev,
                             float* scores_dev, void* stream);

/* ---- retrieval pair selection (csrc/tile_ops.hip) --------------------------------------------------------------
 * thirdparty/hloc/pairs_from_retrieval.py:49-70,108-112: sim = einsum("id,jd->ij", query, db) (global descriptors,
 * fp32 MFMA), invalid entries (self matches; score < min_score when use_min_score) -> -inf, torch.topk(num_select) per
 * query row.  indices [nq][num_select] int32 in descending score order (ties: lowest index), -1 where fewer finite
 * entries exist; values likewise.  sim_scratch: nq * nd floats.  dim must be a multiple of 32 (zero-pad otherwise). */
int dim_op_retrieval_topk(const float* query_dev, int nq, const float* db_dev, int nd, int dim, const unsigned char* invalid_dev, int num_select,
                          float min_score, int use_min_score, float* sim_scratch_dev, int* indices_dev, float* values_dev, void* stream);

/* ---- geometric verification on device (csrc/geom_verify.hip) ----------------------------------------------
 * Replaces the per-pair host call geometric_verification(kpts0[matches[:,0]], kpts1[matches[:,1]], method, threshold,
 * confidence) that follows _match_pairs in the reference (utils/geometric_verification.py:45-179, called at
 * matchers/matcher_base.py:311): a batched fundamental-matrix RANSAC straight on dim_lg_match's device outputs.
 * Inputs: the feature table's keypoints [n_img][cap][2], pair_idx [n_pairs][2] (NULL = slots 2p, 2p+1), matches
 * [n_pairs][nk][2] int64 + n_matches [n_pairs] exactly as dim_lg_match wrote them, 1 <= nk <= 1 << 20.  Tables with
 * nk <= 4096 keep a pair's correspondences in LDS; wider ones are packed once into the scratch buffer and streamed through
 * LDS in chunks.  The estimator and its results are the same on both paths.
 * threshold_px as the reference passes it (gv_threshold x quality scale); iters = number of 7-point hypotheses (the
 * reference's max_iters is 10000); error_type 0 = Sampson distance (USAC / pydegensac family), 1 = symmetric
 * epipolar distance (max of the two point-line distances, cv2.RANSAC); seed makes the sampling reproducible.
 * Outputs: inlier_mask [n_pairs][nk] uint8 (0 beyond n_matches), n_inliers [n_pairs], F [n_pairs][9] fp64 row-major
 * acting on pixel coordinates (x1^T F x0 = 0, scaled to F33 = 1 when possible; zeros when the pair has < 8 matches, in
 * which case every match is an inlier as in geometric_verification.py:107-110).
 * scratch: dim_gv_scratch_bytes_nk(n_pairs, nk) bytes of device memory (the split results, plus the packed points when
 * nk > 4096); dim_gv_scratch_bytes(n_pairs) is that size for nk <= 4096.  The estimator is deterministic and restated in
 * numpy by oracle/geom_ref.py; it is NOT result-identical to cv2's MAGSAC (no two RANSACs are). */
size_t dim_gv_scratch_bytes(int n_pairs);
size_t dim_gv_scratch_bytes_nk(int n_pairs, int nk);
int dim_gv_fundamental(const float* kpts_tab_dev, int cap, const int32_t* pair_idx_dev, const int64_t* matches_dev,
                       const int32_t* n_matches_dev, int nk, int n_pairs, double threshold_px, int iters, int error_type, unsigned seed,
                       void* scratch_dev, size_t scratch_bytes, unsigned char* inlier_mask_dev, int32_t* n_inliers_dev, double* F_dev,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIM_HIP_H */
