// XFeat (thirdparty/accelerated_features/modules/{xfeat,model,interpolator}.py = XFM / XFN / XFI) kernels for gfx950: preparation (resize, channel
// mean, InstanceNorm), the bandwidth-bound stem as direct fp32 convolutions over LDS halo tiles, the head tails, the single-pass NMS / key map and
// the bicubic sparse tail.  The trunk is nhwc_conv.hip's implicit GEMM on the matrix cores (stride 2 and the 8 x 8 unfold operand load included).
// Everything here is fp32 (fp64 for the image statistics) in every mode.  Every reduction has a fixed order; no floating-point atomics.
#include "xfeat_kernels.h"

namespace {

// ATen's upsample_bilinear2d source index with align_corners=False: (dst + 0.5) * (in / out) - 0.5, clamped at 0; second tap clamped at the edge
struct XfTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ XfTap xf_tap(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  float f = ((float)dst + 0.5f) * scale - 0.5f;
  f = f < 0.f ? 0.f : f;
  XfTap t;
  t.i0 = (int)f;
  if (t.i0 > in - 1) t.i0 = in - 1;
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = f - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}

// fixed-order tree over the 256 threads of a workgroup (fp64 pairs)
__device__ __forceinline__ void xf_block_sum2(double& a, double& b, double (*sh)[2]) {
  const int t = threadIdx.x;
  sh[t][0] = a; sh[t][1] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { sh[t][0] += sh[t + o][0]; sh[t][1] += sh[t + o][1]; }
    __syncthreads();
  }
  a = sh[0][0]; b = sh[0][1];
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xf_gray_kernel(const float* __restrict__ image, int C, int in_h, int in_w, float* __restrict__ gray,
                                                      double* __restrict__ partial, int H, int W) {
  __shared__ double sh[256][2];
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  double v = 0.0;
  if (p < H * W) {
    const int y = p / W, x = p % W;
    const XfTap ty = xf_tap(y, in_h, H), tx = xf_tap(x, in_w, W);
    const float* img = image + (size_t)b * in_h * in_w * C;
    float sum = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v00 = img[((size_t)ty.i0 * in_w + tx.i0) * C + c], v01 = img[((size_t)ty.i0 * in_w + tx.i1) * C + c];
      const float v10 = img[((size_t)ty.i1 * in_w + tx.i0) * C + c], v11 = img[((size_t)ty.i1 * in_w + tx.i1) * C + c];
      sum += ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
    }
    const float g = sum / (float)C;
    gray[(size_t)b * H * W + p] = g;
    v = (double)g;
  }
  double s1 = v, s2 = v * v;
  xf_block_sum2(s1, s2, sh);
  if (threadIdx.x == 0) {
    double* dst = partial + ((size_t)b * gridDim.x + blockIdx.x) * 2;
    dst[0] = s1; dst[1] = s2;
  }
}

__global__ __launch_bounds__(256) void xf_stats_kernel(const double* __restrict__ partial, int n_blocks, int n_pixels, double* __restrict__ stats) {
  __shared__ double sh[256][2];
  const int b = blockIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < n_blocks; i += 256) {
    s1 += partial[((size_t)b * n_blocks + i) * 2];
    s2 += partial[((size_t)b * n_blocks + i) * 2 + 1];
  }
  xf_block_sum2(s1, s2, sh);
  if (threadIdx.x == 0) {
    const double mean = s1 / (double)n_pixels;
    double var = s2 / (double)n_pixels - mean * mean;   // biased (InstanceNorm2d, XFN:35)
    if (var < 0.0) var = 0.0;
    stats[b * 2] = mean;
    stats[b * 2 + 1] = 1.0 / sqrt(var + 1e-5);
  }
}

__global__ __launch_bounds__(256) void xf_normalize_kernel(float* __restrict__ plane, const double* __restrict__ stats, int n_pixels, unsigned* sat) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= n_pixels) return;
  const double mean = stats[b * 2], rstd = stats[b * 2 + 1];
  const float v = (float)(((double)plane[(size_t)b * n_pixels + p] - mean) * rstd);
  plane[(size_t)b * n_pixels + p] = v;
  sat_report(sat, fabsf(v));
}

// ---------------------------------------------------------------------------
// Stem.  One workgroup = a 16 x 16 tile of OUTPUT pixels, one thread per pixel and all output channels; inputs staged in LDS with their halo, planar
// per channel; weights are read with wave-uniform addresses (scalar loads).  Zero padding: a halo position outside the map reads 0 — for the fused pair
// that holds for block1.0's OUTPUT (block1.1 pads ITS input, the 4-channel map, with zeros), so positions outside the frame are not convolved.
constexpr int XS_T = 16;
__global__ __launch_bounds__(256) void xf_stem12_kernel(const float* __restrict__ plane, const XfStem w, float* __restrict__ out, int H, int W) {
  constexpr int IN = 2 * XS_T + 3, MID = 2 * XS_T + 1;   // 35 input rows / columns, 33 of the 4-channel map
  __shared__ float sin_[IN][IN + 1];
  __shared__ float smid[4][MID][MID + 1];
  const int b = blockIdx.z, H2 = H / 2, W2 = W / 2;
  const int oy0 = blockIdx.y * XS_T, ox0 = blockIdx.x * XS_T;
  const int my0 = 2 * oy0 - 1, mx0 = 2 * ox0 - 1;         // origin of the 4-channel tile in the full-resolution frame
  const float* src = plane + (size_t)b * H * W;
  for (int i = threadIdx.x; i < IN * IN; i += 256) {
    const int r = i / IN, c = i % IN, y = my0 - 1 + r, x = mx0 - 1 + c;
    sin_[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(size_t)y * W + x] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MID * MID; i += 256) {
    const int r = i / MID, c = i % MID, y = my0 + r, x = mx0 + c;
    const bool ok = y >= 0 && y < H && x >= 0 && x < W;
    float v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) v[t] = sin_[r + t / 3][c + t % 3];
#pragma unroll
    for (int co = 0; co < 4; ++co) {
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) a = fmaf(w.w1[co * 9 + t], v[t], a);
      smid[co][r][c] = ok ? fmaxf(a + w.b1[co], 0.f) : 0.f;
    }
  }
  __syncthreads();
  const int ty = threadIdx.x / XS_T, tx = threadIdx.x % XS_T, oy = oy0 + ty, ox = ox0 + tx;
  float acc[8];
#pragma unroll
  for (int co = 0; co < 8; ++co) acc[co] = 0.f;
  for (int ci = 0; ci < 4; ++ci)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float v = smid[ci][2 * ty + t / 3][2 * tx + t % 3];
      const float* wr = w.w2 + (ci * 9 + t) * 8;
#pragma unroll
      for (int co = 0; co < 8; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
    }
  if (oy < H2 && ox < W2) {
    float* dst = out + (((size_t)b * H2 + oy) * W2 + ox) * 8;
    float4 o0, o1;
    o0.x = fmaxf(acc[0] + w.b2[0], 0.f); o0.y = fmaxf(acc[1] + w.b2[1], 0.f); o0.z = fmaxf(acc[2] + w.b2[2], 0.f); o0.w = fmaxf(acc[3] + w.b2[3], 0.f);
    o1.x = fmaxf(acc[4] + w.b2[4], 0.f); o1.y = fmaxf(acc[5] + w.b2[5], 0.f); o1.z = fmaxf(acc[6] + w.b2[6], 0.f); o1.w = fmaxf(acc[7] + w.b2[7], 0.f);
    *(float4*)dst = o0; *(float4*)(dst + 4) = o1;
  }
}

// 8-channel NHWC input tile with halo into planar LDS: rows y0 + [0, R), columns x0 + [0, R); zeros outside the map
template <int R>
__device__ __forceinline__ void xf_stage8(const float* __restrict__ in, int Hh, int Ww, int y0, int x0, float (*sm)[R][R + 1]) {
  for (int i = threadIdx.x; i < R * R; i += 256) {
    const int r = i / R, c = i % R, y = y0 + r, x = x0 + c;
    float4 u0 = {0.f, 0.f, 0.f, 0.f}, u1 = {0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < Hh && x >= 0 && x < Ww) {
      const float* p = in + ((size_t)y * Ww + x) * 8;
      u0 = *(const float4*)p; u1 = *(const float4*)(p + 4);
    }
    sm[0][r][c] = u0.x; sm[1][r][c] = u0.y; sm[2][r][c] = u0.z; sm[3][r][c] = u0.w;
    sm[4][r][c] = u1.x; sm[5][r][c] = u1.y; sm[6][r][c] = u1.z; sm[7][r][c] = u1.w;
  }
}

__global__ __launch_bounds__(256) void xf_stem3_kernel(const float* __restrict__ in, const XfStem w, float* __restrict__ out, int H2, int W2) {
  constexpr int R = XS_T + 2;
  __shared__ float sm[8][R][R + 1];
  const int b = blockIdx.z, oy0 = blockIdx.y * XS_T, ox0 = blockIdx.x * XS_T;
  xf_stage8<R>(in + (size_t)b * H2 * W2 * 8, H2, W2, oy0 - 1, ox0 - 1, sm);
  __syncthreads();
  const int ty = threadIdx.x / XS_T, tx = threadIdx.x % XS_T, oy = oy0 + ty, ox = ox0 + tx;
  float acc[8];
#pragma unroll
  for (int co = 0; co < 8; ++co) acc[co] = 0.f;
  for (int ci = 0; ci < 8; ++ci)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float v = sm[ci][ty + t / 3][tx + t % 3];
      const float* wr = w.w3 + (ci * 9 + t) * 8;
#pragma unroll
      for (int co = 0; co < 8; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
    }
  if (oy < H2 && ox < W2) {
    float* dst = out + (((size_t)b * H2 + oy) * W2 + ox) * 8;
    float4 o0, o1;
    o0.x = fmaxf(acc[0] + w.b3[0], 0.f); o0.y = fmaxf(acc[1] + w.b3[1], 0.f); o0.z = fmaxf(acc[2] + w.b3[2], 0.f); o0.w = fmaxf(acc[3] + w.b3[3], 0.f);
    o1.x = fmaxf(acc[4] + w.b3[4], 0.f); o1.y = fmaxf(acc[5] + w.b3[5], 0.f); o1.z = fmaxf(acc[6] + w.b3[6], 0.f); o1.w = fmaxf(acc[7] + w.b3[7], 0.f);
    *(float4*)dst = o0; *(float4*)(dst + 4) = o1;
  }
}

__global__ __launch_bounds__(256) void xf_stem4_kernel(const float* __restrict__ in, const float* __restrict__ plane, const XfStem w, float* __restrict__ out,
                                                       int H2, int W2, unsigned* sat) {
  constexpr int R = 2 * XS_T + 1;
  __shared__ float sm[8][R][R + 1];
  const int b = blockIdx.z, H4 = H2 / 2, W4 = W2 / 2, oy0 = blockIdx.y * XS_T, ox0 = blockIdx.x * XS_T;
  xf_stage8<R>(in + (size_t)b * H2 * W2 * 8, H2, W2, 2 * oy0 - 1, 2 * ox0 - 1, sm);
  __syncthreads();
  const int ty = threadIdx.x / XS_T, tx = threadIdx.x % XS_T, oy = oy0 + ty, ox = ox0 + tx;
  float acc[24];
#pragma unroll
  for (int co = 0; co < 24; ++co) acc[co] = 0.f;
  for (int ci = 0; ci < 8; ++ci)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float v = sm[ci][2 * ty + t / 3][2 * tx + t % 3];
      const float* wr = w.w4 + (ci * 9 + t) * 24;
#pragma unroll
      for (int co = 0; co < 24; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
    }
  if (oy >= H4 || ox >= W4) return;
  // skip1 (XFN:40-41): 4 x 4 average of the normalised image (full resolution = 4 x this map), then 1 -> 24 with bias
  const int Wf = 2 * W2;
  const float* ps = plane + ((size_t)b * (2 * H2) + 4 * oy) * Wf + 4 * ox;
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float4 u = *(const float4*)(ps + (size_t)r * Wf);
    sum += u.x; sum += u.y; sum += u.z; sum += u.w;
  }
  const float avg = sum * 0.0625f;
  float* dst = out + (((size_t)b * H4 + oy) * W4 + ox) * 32;
  float track = 0.f;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int co = 4 * q + e;
      o[e] = fmaxf(acc[co] + w.b4[co], 0.f) + (w.skip_w[co] * avg + w.skip_b[co]);
      track = fmaxf(track, fabsf(o[e]));
    }
    float4 u; u.x = o[0]; u.y = o[1]; u.z = o[2]; u.w = o[3];
    *(float4*)(dst + 4 * q) = u;
  }
  const float4 z = {0.f, 0.f, 0.f, 0.f};
  *(float4*)(dst + 24) = z; *(float4*)(dst + 28) = z;
  sat_report(sat, track);
}

// one thread per (pixel, four channels)
__global__ __launch_bounds__(256) void xf_fuse_kernel(const float* __restrict__ x3, const float* __restrict__ x4, const float* __restrict__ x5, float* __restrict__ out,
                                                      int H8, int W8, unsigned* sat) {
  const int item = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (item >= H8 * W8 * 16) return;
  const int p = item >> 4, c = (item & 15) * 4, y = p / W8, x = p % W8;
  const int H16 = H8 / 2, W16 = W8 / 2, H32 = H8 / 4, W32 = W8 / 4;
  auto up = [&](const float* m, int Hl, int Wl) {
    const XfTap ty = xf_tap(y, Hl, H8), tx = xf_tap(x, Wl, W8);
    const float* base = m + (size_t)b * Hl * Wl * 64 + c;
    const float4 v00 = *(const float4*)(base + ((size_t)ty.i0 * Wl + tx.i0) * 64), v01 = *(const float4*)(base + ((size_t)ty.i0 * Wl + tx.i1) * 64);
    const float4 v10 = *(const float4*)(base + ((size_t)ty.i1 * Wl + tx.i0) * 64), v11 = *(const float4*)(base + ((size_t)ty.i1 * Wl + tx.i1) * 64);
    float4 r;
    r.x = ty.l0 * (tx.l0 * v00.x + tx.l1 * v01.x) + ty.l1 * (tx.l0 * v10.x + tx.l1 * v11.x);
    r.y = ty.l0 * (tx.l0 * v00.y + tx.l1 * v01.y) + ty.l1 * (tx.l0 * v10.y + tx.l1 * v11.y);
    r.z = ty.l0 * (tx.l0 * v00.z + tx.l1 * v01.z) + ty.l1 * (tx.l0 * v10.z + tx.l1 * v11.z);
    r.w = ty.l0 * (tx.l0 * v00.w + tx.l1 * v01.w) + ty.l1 * (tx.l0 * v10.w + tx.l1 * v11.w);
    return r;
  };
  const float4 a = *(const float4*)(x3 + ((size_t)b * H8 * W8 + p) * 64 + c), u4 = up(x4, H16, W16), u5 = up(x5, H32, W32);
  float4 o;
  o.x = (a.x + u4.x) + u5.x; o.y = (a.y + u4.y) + u5.y; o.z = (a.z + u4.z) + u5.z; o.w = (a.w + u4.w) + u5.w;
  *(float4*)(out + ((size_t)b * H8 * W8 + p) * 64 + c) = o;
  sat_report(sat, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
}

// ---------------------------------------------------------------------------
// keypoint head tail: one wave per cell, lane c = logit c (its 64 weights in registers), the dustbin logit evaluated by every lane from LDS;
// softmax through wave_max / wave_sum's fixed butterflies; lane c stores pixel (c / 8, c % 8) of the cell (XFM:242-247)
constexpr int XK_CPW = 8;   // cells per wave
__global__ __launch_bounds__(256) void xf_kp_tail_kernel(const float* __restrict__ hid, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ k1h, int H8, int W8) {
  __shared__ float wd[64];
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  if (threadIdx.x < 64) wd[threadIdx.x] = w[64 * 64 + threadIdx.x];
  float wr[64];
#pragma unroll
  for (int k = 0; k < 64; k += 4) {
    const float4 u = *(const float4*)(w + lane * 64 + k);
    wr[k] = u.x; wr[k + 1] = u.y; wr[k + 2] = u.z; wr[k + 3] = u.w;
  }
  const float bc = bias[lane], bd = bias[64];
  __syncthreads();
  const int cell0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * XK_CPW, n_cells = H8 * W8, W = 8 * W8;
  for (int q = 0; q < XK_CPW; ++q) {
    const int cell = cell0 + q;
    if (cell >= n_cells) break;   // (wave-uniform)
    const float* x = hid + ((size_t)b * n_cells + cell) * 64;
    float lc = 0.f, ld = 0.f;
#pragma unroll
    for (int k = 0; k < 64; k += 4) {
      const float4 u = *(const float4*)(x + k);
      lc = fmaf(wr[k], u.x, lc); lc = fmaf(wr[k + 1], u.y, lc); lc = fmaf(wr[k + 2], u.z, lc); lc = fmaf(wr[k + 3], u.w, lc);
      ld = fmaf(wd[k], u.x, ld); ld = fmaf(wd[k + 1], u.y, ld); ld = fmaf(wd[k + 2], u.z, ld); ld = fmaf(wd[k + 3], u.w, ld);
    }
    lc += bc; ld += bd;
    const float m = fmaxf(wave_max(lc), ld);
    const float ec = expf(lc - m), ed = expf(ld - m);
    const float sum = wave_sum(ec) + ed;
    const int cy = cell / W8, cx = cell % W8;
    k1h[((size_t)b * 8 * H8 + 8 * cy + (lane >> 3)) * W + 8 * cx + (lane & 7)] = ec / sum;
  }
}

__global__ __launch_bounds__(256) void xf_dense_tail_kernel(const float* __restrict__ hid, const float* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ feats, float* __restrict__ h1, float* __restrict__ m1, int n_pixels) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pixels) return;
  const float* x = hid + (size_t)p * 64;
  float s = 0.f;
  for (int k = 0; k < 64; k += 4) {
    const float4 u = *(const float4*)(x + k);
    s = fmaf(w[k], u.x, s); s = fmaf(w[k + 1], u.y, s); s = fmaf(w[k + 2], u.z, s); s = fmaf(w[k + 3], u.w, s);
  }
  h1[p] = 1.0f / (1.0f + expf(-(s + bias[0])));
  const float* f = feats + (size_t)p * 64;
  float n2 = 0.f;
  for (int k = 0; k < 64; k += 4) {
    const float4 u = *(const float4*)(f + k);
    n2 = fmaf(u.x, u.x, n2); n2 = fmaf(u.y, u.y, n2); n2 = fmaf(u.z, u.z, n2); n2 = fmaf(u.w, u.w, n2);
  }
  const float n = fmaxf(sqrtf(n2), 1e-12f);
  float* o = m1 + (size_t)p * 64;
  for (int k = 0; k < 64; k += 4) {
    const float4 u = *(const float4*)(f + k);
    float4 r; r.x = u.x / n; r.y = u.y / n; r.z = u.z / n; r.w = u.w / n;
    *(float4*)(o + k) = r;
  }
}

// ---------------------------------------------------------------------------
// grid_sample's source coordinate of integer pixel p (XFI:19,32 with ATen's align_corners=False un-normalisation (g + 1) * (size / 2) - 0.5), in the
// reference's fp32 operation order: `full` = the full-resolution size the grid is normalised with, `size` = the sampled map's size
__device__ __forceinline__ float xf_coord(int p, int full, int size) {
  const float g = 2.0f * ((float)p / (float)(full - 1)) - 1.0f;
  return fmaf(g + 1.0f, (float)size / 2.0f, -0.5f);   // (fused, as torch's CPU builds evaluate it: bit-equal on crafted maps, tests/xfeat_cases.py)
}

__global__ __launch_bounds__(256) void xf_keys_kernel(const float* __restrict__ k1h, const float* __restrict__ h1, float* __restrict__ key, float thr, int H, int W) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= H * W) return;
  const int y = p / W, x = p % W;
  const float* K = k1h + (size_t)b * H * W;
  const float v = K[p];
  float out = 0.f;
  if (v > thr && (x | y) != 0) {
    bool is_max = true;   // v == maxpool5x5(v): no value of the window (padding excluded) is larger
    for (int dy = -2; dy <= 2; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      for (int dx = -2; dx <= 2; ++dx) {
        const int xx = x + dx;
        if (xx >= 0 && xx < W && K[(size_t)yy * W + xx] > v) is_max = false;
      }
    }
    if (is_max) {
      // nearest sample of K1h (half to even, as nearbyint): (W - 1) -> W - 0.5 -> W, outside; 0 -> -0.5 -> -0, pixel 0
      const int nx = (int)nearbyintf(xf_coord(x, W, W)), ny = (int)nearbyintf(xf_coord(y, H, H));
      const float kv = (nx >= 0 && nx < W && ny >= 0 && ny < H) ? K[(size_t)ny * W + nx] : 0.f;
      // bilinear sample of H1, zero padding; ATen's weights and order, nw (s e) + ne (s w) + sw (n e) + se (n w), each addition fused with its product
      // (what torch's CPU builds do: bit-equal to them in tests/xfeat_cases.py's crafted maps and on 3000 random samples of a 128 x 128 map)
      const int H8 = H / 8, W8 = W / 8;
      const float fx = xf_coord(x, W, W8), fy = xf_coord(y, H, H8);
      const float xw = floorf(fx), yn = floorf(fy);
      const float ww = fx - xw, e = 1.0f - ww, n = fy - yn, s = 1.0f - n;
      const int ix = (int)xw, iy = (int)yn;
      const float* R = h1 + (size_t)b * H8 * W8;
      auto at = [&](int yy, int xx) { return (yy >= 0 && yy < H8 && xx >= 0 && xx < W8) ? R[(size_t)yy * W8 + xx] : 0.f; };
      const float hv = fmaf(at(iy + 1, ix + 1), n * ww, fmaf(at(iy + 1, ix), n * e, fmaf(at(iy, ix + 1), s * ww, at(iy, ix) * (s * e))));
      const float k = kv * hv;
      out = k > 0.f ? k : 0.f;
    }
  }
  key[(size_t)b * H * W + p] = out;
}

// ATen's cubic convolution coefficients (A = -0.75) for the four taps around fraction t
__device__ __forceinline__ void xf_cubic(float t, float (&c)[4]) {
  const float A = -0.75f;
  float x = t + 1.0f;
  c[0] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
  c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  x = 1.0f - t;
  c[2] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  x = 2.0f - t;
  c[3] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
}

// one wave per keypoint, lane = channel
__global__ __launch_bounds__(256) void xf_sparse_kernel(const float* __restrict__ m1, const float* __restrict__ kpts_px, const int* __restrict__ n_kpts,
                                                        float* __restrict__ desc, float* __restrict__ kpts_out, int stride, int capacity, int H, int W, float rw, float rh) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (k >= n_kpts[b] || k >= capacity) return;
  const size_t kk = (size_t)b * capacity + k;
  const float pxf = kpts_px[kk * 2], pyf = kpts_px[kk * 2 + 1];
  const int H8 = H / 8, W8 = W / 8;
  const float fx = xf_coord((int)pxf, W, W8), fy = xf_coord((int)pyf, H, H8);
  const float xw = floorf(fx), yn = floorf(fy);
  float cx[4], cy[4];
  xf_cubic(fx - xw, cx); xf_cubic(fy - yn, cy);
  const int ix = (int)xw - 1, iy = (int)yn - 1;
  const float* M = m1 + (size_t)b * H8 * W8 * 64 + lane;
  float o = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int yy = iy + r;
    float row = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int xx = ix + c;
      const float v = (yy >= 0 && yy < H8 && xx >= 0 && xx < W8) ? M[((size_t)yy * W8 + xx) * 64] : 0.f;
      row += v * cx[c];
    }
    o += row * cy[r];
  }
  const float n = fmaxf(sqrtf(wave_sum(o * o)), 1e-12f);   // F.normalize (XFM:93)
  float* out = desc + kk * stride;
  out[lane] = o / n;
  if (lane + 64 < stride) out[lane + 64] = 0.f;
  if (lane == 0) { kpts_out[kk * 2] = pxf * rw; kpts_out[kk * 2 + 1] = pyf * rh; }
}

}  // namespace

int launch_xf_gray(const float* image, int C, int in_h, int in_w, float* gray, double* partial, int batch, int H, int W, hipStream_t s) {
  DIM_REQUIRE(image && gray && partial && (C == 1 || C == 3) && H >= 1 && W >= 1 && H <= in_h && W <= in_w, "xf_gray: bad argument (C %d, %dx%d -> %dx%d)", C, in_h, in_w, H, W);
  hipLaunchKernelGGL(xf_gray_kernel, dim3(xf_prep_blocks(H, W), batch), dim3(256), 0, s, image, C, in_h, in_w, gray, partial, H, W);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_stats(const double* partial, int n_blocks, int n_pixels, double* stats, int batch, hipStream_t s) {
  hipLaunchKernelGGL(xf_stats_kernel, dim3(batch), dim3(256), 0, s, partial, n_blocks, n_pixels, stats);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_normalize(float* plane, const double* stats, int batch, int n_pixels, unsigned* sat, hipStream_t s) {
  hipLaunchKernelGGL(xf_normalize_kernel, dim3(cdiv(n_pixels, 256), batch), dim3(256), 0, s, plane, stats, n_pixels, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_stem12(const float* plane, const XfStem& w, float* out, int batch, int H, int W, hipStream_t s) {
  DIM_REQUIRE(H % 2 == 0 && W % 2 == 0 && H >= 2 && W >= 2, "xf_stem12: %dx%d", H, W);
  hipLaunchKernelGGL(xf_stem12_kernel, dim3(cdiv(W / 2, XS_T), cdiv(H / 2, XS_T), batch), dim3(256), 0, s, plane, w, out, H, W);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_stem3(const float* in, const XfStem& w, float* out, int batch, int H2, int W2, hipStream_t s) {
  hipLaunchKernelGGL(xf_stem3_kernel, dim3(cdiv(W2, XS_T), cdiv(H2, XS_T), batch), dim3(256), 0, s, in, w, out, H2, W2);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_stem4(const float* in, const float* plane, const XfStem& w, float* out, int batch, int H2, int W2, unsigned* sat, hipStream_t s) {
  DIM_REQUIRE(H2 % 2 == 0 && W2 % 4 == 0 && H2 >= 2 && W2 >= 4, "xf_stem4: %dx%d", H2, W2);   // (rows of the full-resolution plane are read as float4)
  hipLaunchKernelGGL(xf_stem4_kernel, dim3(cdiv(W2 / 2, XS_T), cdiv(H2 / 2, XS_T), batch), dim3(256), 0, s, in, plane, w, out, H2, W2, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_fuse(const float* x3, const float* x4, const float* x5, float* out, int batch, int H8, int W8, unsigned* sat, hipStream_t s) {
  DIM_REQUIRE(H8 % 4 == 0 && W8 % 4 == 0 && H8 >= 4 && W8 >= 4, "xf_fuse: %dx%d", H8, W8);
  hipLaunchKernelGGL(xf_fuse_kernel, dim3(cdiv(H8 * W8 * 16, 256), batch), dim3(256), 0, s, x3, x4, x5, out, H8, W8, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_kp_tail(const float* hid, const float* w, const float* bias, float* k1h, int batch, int H8, int W8, hipStream_t s) {
  hipLaunchKernelGGL(xf_kp_tail_kernel, dim3(cdiv(H8 * W8, 4 * XK_CPW), batch), dim3(256), 0, s, hid, w, bias, k1h, H8, W8);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_dense_tail(const float* hid, const float* w, const float* bias, const float* feats, float* h1, float* m1, int n_pixels, hipStream_t s) {
  hipLaunchKernelGGL(xf_dense_tail_kernel, dim3(cdiv(n_pixels, 256)), dim3(256), 0, s, hid, w, bias, feats, h1, m1, n_pixels);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_keys(const float* k1h, const float* h1, float* key, float thr, int batch, int H, int W, hipStream_t s) {
  DIM_REQUIRE(H % 8 == 0 && W % 8 == 0 && H >= 8 && W >= 8, "xf_keys: %dx%d is no multiple of 8", H, W);
  hipLaunchKernelGGL(xf_keys_kernel, dim3(cdiv(H * W, 256), batch), dim3(256), 0, s, k1h, h1, key, thr, H, W);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_xf_sparse(const float* m1, const float* kpts_px, const int* n_kpts, float* desc, float* kpts_out, int stride, int capacity, int batch, int H, int W,
                     float rw, float rh, hipStream_t s) {
  DIM_REQUIRE(stride >= 64 && stride <= 128, "xf_sparse: stride %d", stride);
  hipLaunchKernelGGL(xf_sparse_kernel, dim3(cdiv(capacity, 4), batch), dim3(256), 0, s, m1, kpts_px, n_kpts, desc, kpts_out, stride, capacity, H, W, rw, rh);
  DIM_LAUNCH_CHECK();
  return 0;
}
