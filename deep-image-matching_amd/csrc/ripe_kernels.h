// Launchers of the RIPE extractor's own kernels (ripe.hip).  Reference: thirdparty/RIPE/ripe/models/ripe.py = RPM, backbones/vgg.py = RPV,
// backbones/vgg_utils.py = RPU, backbones/backbone_base.py = RPB, upsampler/hypercolumn_features.py = RPH.  Feature maps are NHWC fp32; the logit /
// heat / key maps are planes [b][H][W].  Everything runs on the caller's stream and never synchronises; every reduction has a fixed order.
#pragma once
#include "dim_kernels.h"

constexpr int RIPE_DW_TILE = 16;   // output pixels per side of one depthwise workgroup
constexpr int RIPE_DW_CG = 32;     // channels of one depthwise workgroup
constexpr int RIPE_NMS_TILE = 16;  // pixels per side of one detection workgroup
constexpr int RIPE_HYPER_DIM = 64 + 128 + 256 + 512;
constexpr int RIPE_DESC_DIM = 256;

// ---- InstanceNorm2d(3) statistics (RPB:22,63: biased variance, eps 1e-5, no affine) ----
// partial [b][ripe_stats_blocks(H, W)][6] = per workgroup and channel the fp64 (sum, sum of squares); stats [b][3][2] = (mean, 1 / sqrt(var + 1e-5)) in fp64
inline int ripe_stats_blocks(int H, int W) { return (H * W + 255) / 256; }
int launch_ripe_stats(const float* image, double* partial, double* stats, int batch, int H, int W, hipStream_t s);
// layers[0] with the normalisation in its operand load: image [b][H][W][3] -> (x - mean) * rstd (fp64, rounded once), zero padding AFTER it, 3 -> 64
// channels, BatchNorm folded into w [27 = (ci, dy, dx)][64] and bias, ReLU.  out [b][H][W][64]
int launch_ripe_conv1(const float* image, const double* stats, const float* w_27x64, const float* bias, float* out, int batch, int H, int W, unsigned* sat,
                      hipStream_t s);

// ---- decoder (RPU:32-102 ConvRefiner) ----
// depthwise 5 x 5 (pad 2) + folded BatchNorm + ReLU: in / out [b][H][W][C], C % 32 == 0, w [25 = (dy, dx)][C], bias [C]; any H, W >= 1
int launch_ripe_dw5x5(const float* in, const float* w_25xc, const float* bias, float* out, int batch, int H, int W, int C, unsigned* sat, hipStream_t s);
// x = x / 1.4 in place over n floats (n % 4 == 0): the second half of (x + x0) / 1.4 (RPU:99-100); the sum is the 1 x 1 convolution's residual input
int launch_ripe_div14(float* x, size_t n, hipStream_t s);
// F.interpolate(bilinear, align_corners=False) of channels [c_off, c_off + C) of in [b][h][w][ld] to out [b][H][W][C] (RPV:96-97)
int launch_ripe_resize_bilinear(const float* in, int ld, int c_off, int C, int batch, int h, int w, float* out, int H, int W, hipStream_t s);
// out [b][n] = (acc ? acc [b][n] : 0) + delta [b][n][ld] channel 0 (RPV:93)
int launch_ripe_logit_add(const float* acc, const float* delta, int ld, float* out, int batch, int n, hipStream_t s);

// ---- detection (RPM:262-267) ----
// key [b][H][W] = heat where heat == its 3 x 3 window maximum (-inf padding: border pixels are eligible, equal neighbours all stay) and heat > thr,
// else 0.  thr >= 0, so a key > 0 marks a candidate (what launch_select_ex / launch_topk expect).
int launch_ripe_nms3(const float* heat, float* key, float thr, int batch, int H, int W, hipStream_t s);
// mapmax [b] = max over the plane; partial: batch * ripe_max_blocks(n) floats
inline int ripe_max_blocks(int n) { return (n + 4095) / 4096; }
int launch_ripe_map_max(const float* heat, float* partial, float* mapmax, int batch, int n, hipStream_t s);

// ---- descriptors (RPH:23-44, RPM:269-283) ----
// rows [b][capacity][960]: per keypoint (x, y) of kpts [b][capacity][2] the bilinear grid_sample (align_corners=True, zero padding) of the four encoder
// maps f[l] [b][h_l][w_l][c_l] (c = 64, 128, 256, 512) at 2 (x, y) / (W - 1, H - 1) - 1, concatenated.  Rows past n_kpts[b] are not written.
struct RipeLevels { const float* f[4]; int h[4], w[4]; };
int launch_ripe_hypercolumn(const RipeLevels& lv, const float* kpts, const int* n_kpts, float* rows, int capacity, int batch, int H, int W, hipStream_t s);
// desc [b][capacity][256] = lin / max(||lin||, 1e-12) (F.normalize), scores [b][capacity] = raw / mapmax[b] (RPM:241-242); rows past n_kpts[b] zero
int launch_ripe_desc_finish(const float* lin, const float* raw_scores, const float* mapmax, const int* n_kpts, float* desc, float* scores, int capacity, int batch,
                            hipStream_t s);
