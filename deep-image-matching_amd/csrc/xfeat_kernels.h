// Launchers of the XFeat kernels (xfeat.hip).  Reference lines: XFM = thirdparty/accelerated_features/modules/xfeat.py, XFN = modules/model.py,
// XFI = modules/interpolator.py.  Feature maps are NHWC fp32; the image planes (normalised image, keypoint heat map, key map) are [b][H][W].
#pragma once
#include "dim_kernels.h"

// ---- preparation (XFM:219-240, XFN:135-136) ----
// gray[b][y][x] = mean over channels of the bilinear resize (align_corners=False, no antialias) of image [b][in_h][in_w][C] to H x W, and per
// (image, workgroup) the fp64 pair (sum, sum of squares) of what it wrote: partial [b][xf_prep_blocks(H, W)][2]
inline int xf_prep_blocks(int H, int W) { return (H * W + 255) / 256; }
int launch_xf_gray(const float* image, int C, int in_h, int in_w, float* gray, double* partial, int batch, int H, int W, hipStream_t s);
// stats [b][2] = (mean, 1 / sqrt(biased variance + 1e-5)) in fp64 from the partials, added up in a fixed order
int launch_xf_stats(const double* partial, int n_blocks, int n_pixels, double* stats, int batch, hipStream_t s);
// InstanceNorm2d(1) in place: plane = (plane - mean) * rstd, evaluated in fp64 and rounded once; `sat`: range guard of the keypoint head's input
int launch_xf_normalize(float* plane, const double* stats, int batch, int n_pixels, unsigned* sat, hipStream_t s);

// ---- stem (XFN:43-48 block1, XFN:40-41 skip1): direct fp32 convolutions over LDS halo tiles, eval-mode BatchNorm folded into weight and bias ----
struct XfStem {
  const float* w1;   // block1.0: [4][9], b1 [4]
  const float* b1;
  const float* w2;   // block1.1: [4 ci * 9 tap][8 co], b2 [8]
  const float* b2;
  const float* w3;   // block1.2: [8 * 9][8], b3 [8]
  const float* b3;
  const float* w4;   // block1.3: [8 * 9][24], b4 [24]
  const float* b4;
  const float* skip_w;   // skip1.1: [24], [24]
  const float* skip_b;
};
// block1.0 (1 -> 4) and block1.1 (4 -> 8, stride 2) in one kernel: the 4-channel full-resolution map lives in LDS only.  out [b][H/2][W/2][8]
int launch_xf_stem12(const float* plane, const XfStem& w, float* out, int batch, int H, int W, hipStream_t s);
// block1.2 (8 -> 8) on the half-resolution map [b][H2][W2][8]
int launch_xf_stem3(const float* in, const XfStem& w, float* out, int batch, int H2, int W2, hipStream_t s);
// block1.3 (8 -> 24, stride 2) with skip1 (4 x 4 average of the normalised image, 1 -> 24 with bias) added behind the ReLU: out [b][H2/2][W2/2][32]
// (channels 24..31 zero); `sat`: range guard of block2's input
int launch_xf_stem4(const float* in, const float* plane, const XfStem& w, float* out, int batch, int H2, int W2, unsigned* sat, hipStream_t s);

// ---- trunk: launch_nhwc_conv (nhwc_conv.h) ----
// out = x3 + up(x4) + up(x5), bilinear with align_corners=False (XFN:146-148); 64 channels; `sat`: range guard of block_fusion's input
int launch_xf_fuse(const float* x3, const float* x4, const float* x5, float* out, int batch, int H8, int W8, unsigned* sat, hipStream_t s);

// ---- head tails ----
// keypoint head: logits = hid[cell][0..64) . w [65][64] + b, softmax over the 65, dustbin dropped, cell-major depth-to-space (XFM:242-247): K1h [b][8 H8][8 W8]
int launch_xf_kp_tail(const float* hid, const float* w, const float* bias, float* k1h, int batch, int H8, int W8, hipStream_t s);
// H1 = sigmoid(hid . w + b) (XFN:82-83), M1 = feats / max(|feats|, 1e-12) over the 64 channels (XFM:70)
int launch_xf_dense_tail(const float* hid, const float* w, const float* bias, const float* feats, float* h1, float* m1, int n_pixels, hipStream_t s);

// ---- selection and the sparse tail ----
// key[b][y][x] = K1h * bilinear(H1) where K1h is a 5 x 5 window maximum above `thr` (ONE pass, equal values all kept: XFM:249-254), else 0.  Both factors
// go through the reference's samplers (XFI: grid 2 p / (W - 1, H - 1) - 1, align_corners=False, zero padding): the nearest sample of the last row / column
// falls outside the map (key 0); pixel (0, 0) is the padding position (XFM:80, key 0).  Keys <= 0 are stored as 0: "not a candidate".
int launch_xf_keys(const float* k1h, const float* h1, float* key, float thr, int batch, int H, int W, hipStream_t s);
// bicubic (A = -0.75, zero padding) sample of M1 [b][H/8][W/8][64] at the selected pixels, L2-normalised: desc [b][cap][stride] (columns past 64 zero);
// kpts_out = pixel * (rw, rh) (XFM:90-96)
int launch_xf_sparse(const float* m1, const float* kpts_px, const int* n_kpts, float* desc, float* kpts_out, int stride, int capacity, int batch, int H, int W,
                     float rw, float rh, hipStream_t s);
