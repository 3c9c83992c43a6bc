// Launchers of the ALIKE kernels (alike.hip).  All tensors NHWC fp32; reference lines are thirdparty/alike/{alnet,alike,soft_detect}.py.
// The encoder / aggregation convolutions (alnet.py:27-30, 68-84, 166-169) are launch_nhwc_conv (nhwc_conv.h).
#pragma once
#include "dim_kernels.h"

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
