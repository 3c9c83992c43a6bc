// Launchers of the ALIKE kernels (alike.hip).  All tensors NHWC fp32; reference lines are thirdparty/alike/{alnet,alike,soft_detect}.py.
#pragma once
#include "dim_kernels.h"

inline int ak_pad16(int c) { return (c + 15) / 16 * 16; }
inline int ak_pad32(int c) { return (c + 31) / 32 * 32; }

// One encoder / aggregation convolution with eval-mode BatchNorm folded in (alnet.py:27-30, 68-84, 166-169):
//   out[b][y][x][co] = act( sum_{tap,ci} in[b][y+dy][x+dx][ci] w[tap*cin_pad+ci][co] + sum_ci in2[b][y][x][ci] w[taps*cin_pad+ci][co] + bias[co] )
// zero padding; taps = 9 (3x3) or 1.  in2 (optional) is the ResBlock's identity input: its 1x1 `downsample` rides in the same
// product as extra K rows, the BatchNorm scale is folded into the 3x3 rows, bias = BatchNorm bias + downsample bias.
// img3: `in` is the unpadded [b][in_h][in_w][3] image; everything at or past in_h / in_w reads as the zero padding of alike.py:105-113.
// pool = 2 | 4: the max-pooled copy of the activated map goes to `pooled` as well ([b][H/pool][W/pool][out_c]; H, W multiples of pool).
// Channel strides: cin_pad / cin2_pad / out_c are multiples of 16 (padding channels hold zeros); the weights' n_pad is a multiple of 32.
struct AkConv {
  const float* in = nullptr; int cin_pad = 16; int taps = 9;
  const float* in2 = nullptr; int cin2_pad = 0;
  int img3 = 0, in_h = 0, in_w = 0;
  const SplitWeights* wx = nullptr;   // fp16x3: split_weights(K, N, n_pad, 2) of the [K][N] operand
  const float* w32 = nullptr;         // fp32: the same operand [K][n_pad]
  const float* bias = nullptr;        // [n_pad]
  int n_pad = 32;
  float* out = nullptr; int out_c = 16;
  float* pooled = nullptr; int pool = 0;
  int relu = 1;
  int batch = 1, H = 0, W = 0;
  unsigned* sat = nullptr;            // fp16x3 range guard of the stored activations
};
int launch_ak_conv(const AkConv& a, bool x3, hipStream_t s);

// sources of the never materialised dim-channel map x1234 (alnet.py:166-173) on the padded frame Hp x Wp: x1 ([..][c1p]) with conv1
// (w1 [c1p][q], bias-free, ReLU) evaluated per pixel, f2 / f3 / f4 = relu(conv_g x_g) ([..][fq] at 1/2, 1/8, 1/32) interpolated with align_corners=True
struct AkFeat { const float *x1, *f2, *f3, *f4, *w1; int Hp, Wp, c1p, q, fq; };

// q_g[pixel] = w_s[0..q) . f_g[pixel][0..q): the score row of convhead2 applied BEFORE the up-sampling (one channel at the level's resolution)
int launch_ak_project(const float* f, int fq, int q, const float* ws, float* out, int n_pixels, hipStream_t s);
// single-head score map (alnet.py:178-181 on the crop alike.py:119-121): sigmoid( w_s[0:q] . relu(conv1 x1) + up2(q2) + up8(q3) + up32(q4) ), [b][H][W]
int launch_ak_score(const AkFeat& F, const float* ws, const float* q2, const float* q3, const float* q4, float* score, int batch, int H, int W, hipStream_t s);
// rows of x1234: band form (keypoints == nullptr): row r of image b = pixel (y0 + r / W, r % W), r < n_rows;
// keypoint form: row 4 k + c = corner c (x0 + (c & 1), y0 + (c >> 1)) of keypoint k's grid_sample cell (soft_detect.py:55-62), rows of corners outside H x W are zero.
// X: [b][rows_cap][ldx]
int launch_ak_rows(const AkFeat& F, const float* kpts_norm, const int* n_kpts, int capacity, int y0, int n_rows, float* X, int ldx, long long strideX,
                   int batch, int H, int W, unsigned* sat, hipStream_t s);
// alike-l: score[b][y0*W + r] = sigmoid( w_s . hid[b][r][0..dim) ) for r < n_rows
int launch_ak_contract(const float* hid, int ldh, long long strideH, const float* ws, int dim, float* score, int y0, int n_rows, int batch, int H, int W, hipStream_t s);
// soft_detect.py:105-108: rows / columns [0, 3) and [h - 2, h) of the NMS map cleared
int launch_ak_border(float* nms, int batch, int H, int W, hipStream_t s);
// sample_descriptor (soft_detect.py:55-69) on the four corner rows D (image b at b * strideD, rows [4 k + c][ldd]): L2-normalise each corner (alike.py:125), blend with the
// bilinear weights, L2-normalise; desc [b][cap][stride], columns [dim, stride) zero; rows at or past n_kpts[b] untouched
int launch_ak_desc_blend(const float* D, int ldd, long long strideD, const float* kpts_norm, const int* n_kpts, float* desc, int dim, int stride, int capacity, int batch,
                         int H, int W, hipStream_t s);
