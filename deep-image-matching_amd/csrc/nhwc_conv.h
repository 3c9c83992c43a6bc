// The implicit-GEMM NHWC convolution of the small networks (ALIKE's encoder / aggregation, XFeat's trunk; nhwc_conv.hip) and its layer upload.
#pragma once
#include <vector>

#include "dim_kernels.h"

inline int dim_pad16(int c) { return (c + 15) / 16 * 16; }
inline int dim_pad32(int c) { return (c + 31) / 32 * 32; }

// One convolution, eval-mode BatchNorm folded into weight and bias by the caller:
//   out[b][y][x][co] = act( sum_{tap,ci} in[b][stride y + dy][stride x + dx][ci] w[tap * cin_pad + ci][co] + sum_ci in2[b][y][x][ci] w[taps * cin_pad + ci][co] + bias[co] )
// taps = 9 (3x3, dy, dx in -1..1) or 1; every input position outside in_h x in_w reads as zero.  out is [b][H][W][out_c].
// in: [b][in_h][in_w][cin_pad];
//     img3: the [b][in_h][in_w][3] image (cin_pad = 16), in_h <= H and in_w <= W allowed: what lies past the image is the frame's zero padding (alike.py:105-113);
//     unfold8: the plane [b][8 H][8 W] read as its 64-channel 8 x 8 unfolding, channel = 8 dy + dx (XFeat model.py:113-120); taps = 1, cin_pad = 64.
// in2 (optional, [b][H][W][cin2_pad]): extra K rows at output resolution (ALIKE's ResBlock identity: its 1x1 `downsample` rides in the same product).
// pool = 2 | 4: the max-pooled copy of the activated map goes to `pooled` as well ([b][H/pool][W/pool][out_c]; H, W multiples of pool).
// Channel strides: cin_pad / cin2_pad / out_c are multiples of 16 (padding channels hold zeros, and are stored as zeros); the weights' n_pad is a multiple of 32.
struct NhwcConv {
  const float* in = nullptr; int cin_pad = 16, taps = 9, stride = 1, in_h = 0, in_w = 0, img3 = 0, unfold8 = 0;
  const float* in2 = nullptr; int cin2_pad = 0;
  const SplitWeights* wx = nullptr;   // fp16x3: split_weights(K, N, n_pad, 2) of the [K][N] operand
  const float* w32 = nullptr;         // fp32 MFMA: the same operand [K][n_pad]
  const float* bias = nullptr;        // [n_pad]
  int n_pad = 32;
  float* out = nullptr; int out_c = 16;
  float* pooled = nullptr; int pool = 0;
  int relu = 1;
  int batch = 1, H = 0, W = 0;        // output size
  unsigned* sat = nullptr;            // fp16x3 range guard of the stored activations
};
// x3: fp16x3 on v_mfma_f32_32x32x16_f16 (wx), else fp32 MFMA (w32)
int launch_nhwc_conv(const NhwcConv& a, bool x3, hipStream_t s);

// one layer in kernel layout: the [K = taps * cin_pad + cin2_pad][N] operand split for the matrix cores and as fp32 [K][n_pad], bias [n_pad]
struct NhwcConvLayer {
  SplitWeights wx; float* w32 = nullptr; float* bias = nullptr;
  int cin_pad = 16, cin2_pad = 0, taps = 9, stride = 1, n_pad = 32, out_c = 16, relu = 1;
};
// OIHW conv weight (co x ci x k x k, optionally scaled per output channel) into rows [row0 + tap * cin_pad + ci] of a [K][N] operand
void nhwc_conv_pack_oihw(std::vector<float>& kn, int N, int row0, const float* w, int co, int ci, int k, int cin_pad, const std::vector<double>* scale);
// uploads the [K][N] operand in both forms and the bias; sets n_pad / out_c.  For create functions: -1 on failure (DIM_TRY)
int nhwc_conv_upload(DimHandleBase* hb, NhwcConvLayer* L, const std::vector<float>& kn, int K, int N, const std::vector<float>& bias);
