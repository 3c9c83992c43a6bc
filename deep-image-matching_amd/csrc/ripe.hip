// RIPE (thirdparty/RIPE/ripe: models/ripe.py = RPM, models/backbones/{vgg,vgg_utils,backbone_base}.py = RPV / RPU / RPB,
// models/upsampler/hypercolumn_features.py = RPH) kernels for gfx950, around the VGG19-BN convolutions (conv_x6.hip) and the 1 x 1 convolutions (gemm_x6.hip):
//
//   ripe_stats_*            InstanceNorm2d(3) statistics: fp64 sum / sum of squares per image and channel, two fixed-order stages
//   ripe_conv1_kernel       layers[0] (3 -> 64) with the normalisation in its operand load, BatchNorm folded, ReLU: fp32 FMAs, 27 products per output
//   ripe_dw5x5_kernel       the decoder's depthwise 5 x 5 + folded BatchNorm + ReLU over an LDS halo tile per 32-channel group
//   ripe_div14_kernel       x / 1.4 of the refiner's residual
//   ripe_resize_kernel      bilinear resize (align_corners=False) to an arbitrary size of a channel range of a strided NHWC tensor
//   ripe_logit_add_kernel   running logit map + channel 0 of a refiner's output
//   ripe_nms3_kernel        3 x 3 window maximum + threshold -> key map
//   ripe_max_*              map maximum in two stages
//   ripe_hyper_kernel       hypercolumn rows of the selected keypoints (grid_sample, align_corners=True, zero padding)
//   ripe_desc_finish_kernel F.normalize of the 256-d rows, scores / map maximum
//
// Everything here is fp32 (fp64 for the image statistics) in every arithmetic mode.  No floating-point atomics: a result depends on the image alone.
#include <math.h>

#include "ripe_kernels.h"

namespace {

// fixed-order tree over the 256 threads of a workgroup, six fp64 values
__device__ __forceinline__ void ripe_block_sum6(double (&v)[6], double (*sh)[6]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 6; ++k) sh[t][k] = v[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < 6; ++k) sh[t][k] += sh[t + o][k];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = sh[0][k];
}

__global__ __launch_bounds__(256) void ripe_stats_partial_kernel(const float* __restrict__ image, double* __restrict__ partial, int n_pixels) {
  __shared__ double sh[256][6];
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (p < n_pixels) {
    const float* px = image + ((size_t)b * n_pixels + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = (double)px[c];
      v[2 * c] = x; v[2 * c + 1] = x * x;
    }
  }
  ripe_block_sum6(v, sh);
  if (threadIdx.x < 6) partial[((size_t)b * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = v[threadIdx.x];
}

__global__ __launch_bounds__(256) void ripe_stats_finish_kernel(const double* __restrict__ partial, int n_blocks, int n_pixels, double* __restrict__ stats) {
  __shared__ double sh[256][6];
  const int b = blockIdx.x;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n_blocks; i += 256)
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += partial[((size_t)b * n_blocks + i) * 6 + k];
  ripe_block_sum6(v, sh);
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    const double mean = v[2 * c] / (double)n_pixels;
    double var = v[2 * c + 1] / (double)n_pixels - mean * mean;   // biased (InstanceNorm2d)
    if (var < 0.0) var = 0.0;
    stats[(b * 3 + c) * 2] = mean;
    stats[(b * 3 + c) * 2 + 1] = 1.0 / sqrt(var + 1e-5);
  }
}

// 64 pixels x 4 groups of 16 output channels per workgroup (netvlad.hip's conv1_1 with another operand load)
__global__ __launch_bounds__(256) void ripe_conv1_kernel(const float* __restrict__ image, const double* __restrict__ stats, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out, int H, int W, unsigned* sat) {
  __shared__ float wl[27 * 64];
  __shared__ float bl[64];
  const int t = threadIdx.x, b = blockIdx.y;
  for (int i = t; i < 27 * 64; i += 256) wl[i] = w[i];
  if (t < 64) bl[t] = bias[t];
  __syncthreads();
  const int p = blockIdx.x * 64 + (t >> 2), cg = t & 3;
  if (p >= H * W) return;
  const int y = p / W, x = p - y * W;
  const float* img = image + (size_t)b * H * W * 3;
  float in27[27];
  bool bad = false;
#pragma unroll
  for (int ci = 0; ci < 3; ++ci) {
    const double mean = stats[(b * 3 + ci) * 2], rstd = stats[(b * 3 + ci) * 2 + 1];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int gy = y + dy - 1, gx = x + dx - 1;
        float v = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
          const float px = img[((size_t)gy * W + gx) * 3 + ci];
          bad |= !(px - px == 0.0f);   // a non-finite pixel: reported where a guard counter is given
          v = (float)(((double)px - mean) * rstd);
        }
        in27[ci * 9 + dy * 3 + dx] = v;
      }
  }
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int j = 0; j < 27; ++j)
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = fmaf(in27[j], wl[j * 64 + cg * 16 + c], acc[c]);
  float vmax = 0.0f;
  float* o = out + ((size_t)b * H * W + p) * 64 + cg * 16;
#pragma unroll
  for (int c = 0; c < 16; c += 4) {
    float4 v;
    v.x = fmaxf(acc[c] + bl[cg * 16 + c], 0.0f); v.y = fmaxf(acc[c + 1] + bl[cg * 16 + c + 1], 0.0f);
    v.z = fmaxf(acc[c + 2] + bl[cg * 16 + c + 2], 0.0f); v.w = fmaxf(acc[c + 3] + bl[cg * 16 + c + 3], 0.0f);
    vmax = fmaxf(vmax, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    *(float4*)(o + c) = v;
  }
  sat_report(sat, bad ? INFINITY : vmax);
}

// ---- depthwise 5 x 5 ---------------------------------------------------------------------------------------------------------------------
// Workgroup (tile, channel group, image): a 16 x 16 tile of output pixels x 32 channels.  The 20 x 20 halo of the group is staged in LDS as float4s
// ([position][8 quads]: the 8 lanes of a pixel read 128 contiguous bytes of the map, a wave 8 neighbouring pixels); positions outside the map hold the
// zero padding, so a window wider than the map needs no other case.  Thread (quad q, slot ps): channels 4 q .. 4 q + 3 of column ps & 15, rows
// (ps >> 4) + 2 i; its 25 taps x 4 channels stay in registers (100 VGPRs).
constexpr int DW_HALO = RIPE_DW_TILE + 4, DW_Q = RIPE_DW_CG / 4;
__global__ __launch_bounds__(256) void ripe_dw5x5_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ out, int H, int W, int C, int tiles_x, unsigned* sat) {
  __shared__ float4 tile[DW_HALO * DW_HALO * DW_Q];
  const int t = threadIdx.x, q = t & (DW_Q - 1), ps = t >> 3;
  const int ty0 = (blockIdx.x / tiles_x) * RIPE_DW_TILE, tx0 = (blockIdx.x % tiles_x) * RIPE_DW_TILE;
  const int c0 = blockIdx.y * RIPE_DW_CG + q * 4, b = blockIdx.z;
  const float* ib = in + (size_t)b * H * W * C;
  for (int i = ps; i < DW_HALO * DW_HALO; i += 256 / DW_Q) {
    const int hy = i / DW_HALO, hx = i - hy * DW_HALO, gy = ty0 + hy - 2, gx = tx0 + hx - 2;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *(const float4*)(ib + ((size_t)gy * W + gx) * C + c0);
    tile[i * DW_Q + q] = v;
  }
  float4 wv[25];
#pragma unroll
  for (int k = 0; k < 25; ++k) wv[k] = *(const float4*)(w + (size_t)k * C + c0);
  const float4 bv = *(const float4*)(bias + c0);
  __syncthreads();
  const int px = ps & 15, r0 = ps >> 4, gx = tx0 + px;
  float* ob = out + (size_t)b * H * W * C;
  float vmax = 0.0f;
#pragma unroll 1
  for (int i = 0; i < RIPE_DW_TILE / 2; ++i) {
    const int py = r0 + 2 * i, gy = ty0 + py;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const float4 v = tile[((py + dy) * DW_HALO + px + dx) * DW_Q + q], k = wv[dy * 5 + dx];
        acc.x = fmaf(v.x, k.x, acc.x); acc.y = fmaf(v.y, k.y, acc.y); acc.z = fmaf(v.z, k.z, acc.z); acc.w = fmaf(v.w, k.w, acc.w);
      }
    if (gy < H && gx < W) {
      float4 o;
      o.x = fmaxf(acc.x + bv.x, 0.0f); o.y = fmaxf(acc.y + bv.y, 0.0f); o.z = fmaxf(acc.z + bv.z, 0.0f); o.w = fmaxf(acc.w + bv.w, 0.0f);
      vmax = fmaxf(vmax, fmaxf(fmaxf(o.x, o.y), fmaxf(o.z, o.w)));
      *(float4*)(ob + ((size_t)gy * W + gx) * C + c0) = o;
    }
  }
  sat_report(sat, vmax);
}

__global__ __launch_bounds__(256) void ripe_div14_kernel(float* __restrict__ x, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 v = ((float4*)x)[i];
  v.x /= 1.4f; v.y /= 1.4f; v.z /= 1.4f; v.w /= 1.4f;
  ((float4*)x)[i] = v;
}

// ATen's upsample_bilinear2d source index with align_corners=False: (dst + 0.5) * (in / out) - 0.5, clamped at 0; second tap clamped at the edge
struct RipeTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ RipeTap ripe_tap(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  float f = ((float)dst + 0.5f) * scale - 0.5f;
  f = f < 0.f ? 0.f : f;
  RipeTap t;
  t.i0 = (int)f;
  if (t.i0 > in - 1) t.i0 = in - 1;
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = f - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}

// one thread per output element, channel fastest
__global__ __launch_bounds__(256) void ripe_resize_kernel(const float* __restrict__ in, int ld, int c_off, int C, int h, int w, float* __restrict__ out, int H,
                                                          int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // i = ((image * H + y) * W + x) * C + c
  if (i >= n) return;
  const int c = (int)(i % C);
  const size_t p = i / C;
  const int x = (int)(p % W);
  const size_t r = p / W;
  const int y = (int)(r % H);
  const size_t b = r / H;
  const RipeTap ty = ripe_tap(y, h, H), tx = ripe_tap(x, w, W);
  const float* src = in + b * h * w * ld + c_off + c;
  const float v00 = src[((size_t)ty.i0 * w + tx.i0) * ld], v01 = src[((size_t)ty.i0 * w + tx.i1) * ld];
  const float v10 = src[((size_t)ty.i1 * w + tx.i0) * ld], v11 = src[((size_t)ty.i1 * w + tx.i1) * ld];
  // fused multiply-adds: two roundings per blend instead of three
  const float top = fmaf(tx.l1, v01, tx.l0 * v00), bot = fmaf(tx.l1, v11, tx.l0 * v10);
  out[i] = fmaf(ty.l1, bot, ty.l0 * top);
}

__global__ __launch_bounds__(256) void ripe_logit_add_kernel(const float* __restrict__ acc, const float* __restrict__ delta, int ld, float* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = (acc ? acc[i] : 0.0f) + delta[i * ld];
}

// ---- detection -----------------------------------------------------------------------------------------------------------------------------
// one thread per pixel of a 16 x 16 tile; the eight neighbours come from the cache hierarchy (a 1-channel plane: 4 bytes per pixel)
__global__ __launch_bounds__(256) void ripe_nms3_kernel(const float* __restrict__ heat, float* __restrict__ key, float thr, int H, int W, int tiles_x) {
  const int t = threadIdx.x;
  const int y = (blockIdx.x / tiles_x) * RIPE_NMS_TILE + (t >> 4), x = (blockIdx.x % tiles_x) * RIPE_NMS_TILE + (t & 15);
  if (y >= H || x >= W) return;
  const float* hb = heat + (size_t)blockIdx.y * H * W;
  const float v = hb[(size_t)y * W + x];
  float m = v;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int gy = y + dy, gx = x + dx;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) m = fmaxf(m, hb[(size_t)gy * W + gx]);
    }
  key[(size_t)blockIdx.y * H * W + (size_t)y * W + x] = (v == m && v > thr) ? v : 0.0f;
}

__device__ __forceinline__ float ripe_block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__global__ __launch_bounds__(256) void ripe_max_partial_kernel(const float* __restrict__ heat, float* __restrict__ partial, int n) {
  __shared__ float red[4];
  const float* hb = heat + (size_t)blockIdx.y * n;
  float m = -INFINITY;
  for (int i = blockIdx.x * 4096 + threadIdx.x; i < min(n, (int)(blockIdx.x + 1) * 4096); i += 256) m = fmaxf(m, hb[i]);
  m = ripe_block_max(m, red);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
}
__global__ __launch_bounds__(256) void ripe_max_finish_kernel(const float* __restrict__ partial, int n_blocks, float* __restrict__ mapmax) {
  __shared__ float red[4];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < n_blocks; i += 256) m = fmaxf(m, partial[(size_t)blockIdx.x * n_blocks + i]);
  m = ripe_block_max(m, red);
  if (threadIdx.x == 0) mapmax[blockIdx.x] = m;
}

// ---- descriptors ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per keypoint, thread t = channel quads t, t + 256 (960 / 4 = 240 quads: one round).  ATen's grid_sampler_2d (CPU, float):
// g = 2 (p / (size - 1)) - 1 (RPH:23-24, fp32), unnormalised as (g + 1) * ((size_l - 1) / 2); corners floor / floor + 1 with weights
// (1 - dx)(1 - dy), dx (1 - dy), (1 - dx) dy, dx dy added in that order; a corner outside the level contributes zero.
__global__ __launch_bounds__(256) void ripe_hyper_kernel(const RipeLevels lv, const float* __restrict__ kpts, const int* __restrict__ n_kpts,
                                                         float* __restrict__ rows, int capacity, int H, int W) {
  const int i = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  if (i >= n_kpts[b] || t >= RIPE_HYPER_DIM / 4) return;
  const int l = t < 16 ? 0 : (t < 48 ? 1 : (t < 112 ? 2 : 3));
  const int cbase = l == 0 ? 0 : (l == 1 ? 64 : (l == 2 ? 192 : 448)), C = 64 << l;
  const int c = t * 4 - cbase;
  const float kx = kpts[((size_t)b * capacity + i) * 2], ky = kpts[((size_t)b * capacity + i) * 2 + 1];
  const float gx = 2.0f * (kx / (float)(W - 1)) - 1.0f, gy = 2.0f * (ky / (float)(H - 1)) - 1.0f;
  const int h = lv.h[l], w = lv.w[l];
  const float fx = (gx + 1.0f) * ((float)(w - 1) / 2.0f), fy = (gy + 1.0f) * ((float)(h - 1) / 2.0f);
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float dx = fx - x0f, dy = fy - y0f, ex = 1.0f - dx, sy = 1.0f - dy;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float wt[4] = {sy * ex, sy * dx, dy * ex, dy * dx};
  const float* f = lv.f[l] + (size_t)b * h * w * C + c;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cx >= 0 && cx < w && cy >= 0 && cy < h) v = *(const float4*)(f + ((size_t)cy * w + cx) * C);
    if (k == 0) { acc.x = v.x * wt[0]; acc.y = v.y * wt[0]; acc.z = v.z * wt[0]; acc.w = v.w * wt[0]; }
    else { acc.x += v.x * wt[k]; acc.y += v.y * wt[k]; acc.z += v.z * wt[k]; acc.w += v.w * wt[k]; }
  }
  *(float4*)(rows + ((size_t)b * capacity + i) * RIPE_HYPER_DIM + t * 4) = acc;
}

// one wave per keypoint: lane = channels 4 lane .. 4 lane + 3 of the 256
__global__ __launch_bounds__(256) void ripe_desc_finish_kernel(const float* __restrict__ lin, const float* __restrict__ raw, const float* __restrict__ mapmax,
                                                               const int* __restrict__ n_kpts, float* __restrict__ desc, float* __restrict__ scores, int capacity) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (i >= capacity) return;
  const size_t row = (size_t)b * capacity + i;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool live = i < n_kpts[b];
  if (live) {
    v = *(const float4*)(lin + row * RIPE_DESC_DIM + lane * 4);
    float q = v.x * v.x;
    q = fmaf(v.y, v.y, q); q = fmaf(v.z, v.z, q); q = fmaf(v.w, v.w, q);
    const float den = fmaxf(sqrtf(wave_sum(q)), 1e-12f);
    v.x /= den; v.y /= den; v.z /= den; v.w /= den;
  }
  *(float4*)(desc + row * RIPE_DESC_DIM + lane * 4) = v;
  if (lane == 0) scores[row] = live ? raw[row] / mapmax[b] : 0.0f;
}
}  // namespace

int launch_ripe_stats(const float* image, double* partial, double* stats, int batch, int H, int W, hipStream_t s) {
  DIM_REQUIRE((long long)H * W <= 0x7fffffffLL / 64, "ripe stats: image %d x %d too large", H, W);
  if (batch <= 0 || H <= 0 || W <= 0) return 0;
  const int nblk = ripe_stats_blocks(H, W);
  hipLaunchKernelGGL(ripe_stats_partial_kernel, dim3(nblk, batch), dim3(256), 0, s, image, partial, H * W);
  DIM_LAUNCH_CHECK();
  hipLaunchKernelGGL(ripe_stats_finish_kernel, dim3(batch), dim3(256), 0, s, (const double*)partial, nblk, H * W, stats);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_conv1(const float* image, const double* stats, const float* w_27x64, const float* bias, float* out, int batch, int H, int W, unsigned* sat,
                      hipStream_t s) {
  DIM_REQUIRE((long long)H * W <= 0x7fffffffLL / 64, "ripe conv1: image %d x %d too large", H, W);
  if (batch <= 0 || H <= 0 || W <= 0) return 0;
  hipLaunchKernelGGL(ripe_conv1_kernel, dim3(cdiv(H * W, 64), batch), dim3(256), 0, s, image, stats, w_27x64, bias, out, H, W, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_dw5x5(const float* in, const float* w_25xc, const float* bias, float* out, int batch, int H, int W, int C, unsigned* sat, hipStream_t s) {
  DIM_REQUIRE(C > 0 && C % RIPE_DW_CG == 0 && C / RIPE_DW_CG <= 65535, "ripe dw5x5: %d channels (a multiple of %d)", C, RIPE_DW_CG);
  DIM_REQUIRE(batch <= 65535, "ripe dw5x5: batch %d", batch);
  if (batch <= 0 || H <= 0 || W <= 0) return 0;
  const int tx = cdiv(W, RIPE_DW_TILE), ty = cdiv(H, RIPE_DW_TILE);
  hipLaunchKernelGGL(ripe_dw5x5_kernel, dim3(tx * ty, C / RIPE_DW_CG, batch), dim3(256), 0, s, in, w_25xc, bias, out, H, W, C, tx, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_div14(float* x, size_t n, hipStream_t s) {
  DIM_REQUIRE(n % 4 == 0 && (n / 4 + 255) / 256 <= 0x7fffffffull, "ripe div14: %zu elements", n);
  if (n == 0) return 0;
  hipLaunchKernelGGL(ripe_div14_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, x, n / 4);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_resize_bilinear(const float* in, int ld, int c_off, int C, int batch, int h, int w, float* out, int H, int W, hipStream_t s) {
  DIM_REQUIRE(C >= 1 && c_off >= 0 && c_off + C <= ld, "ripe resize: channels [%d, %d) of %d", c_off, c_off + C, ld);
  DIM_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1, "ripe resize: %d x %d -> %d x %d", h, w, H, W);
  const size_t n = (size_t)batch * H * W * C;
  if (batch <= 0) return 0;
  DIM_REQUIRE((n + 255) / 256 <= 0x7fffffffull, "ripe resize: %zu elements exceed one grid", n);
  hipLaunchKernelGGL(ripe_resize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, ld, c_off, C, h, w, out, H, W, n);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_logit_add(const float* acc, const float* delta, int ld, float* out, int batch, int n, hipStream_t s) {
  const size_t total = (size_t)batch * n;
  if (batch <= 0 || n <= 0) return 0;
  hipLaunchKernelGGL(ripe_logit_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, acc, delta, ld, out, total);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_nms3(const float* heat, float* key, float thr, int batch, int H, int W, hipStream_t s) {
  DIM_REQUIRE(thr >= 0.0f, "ripe nms3: threshold %g below 0 (a key of 0 marks a pixel that is no candidate)", (double)thr);
  DIM_REQUIRE(batch <= 65535, "ripe nms3: batch %d", batch);
  if (batch <= 0 || H <= 0 || W <= 0) return 0;
  const int tx = cdiv(W, RIPE_NMS_TILE), ty = cdiv(H, RIPE_NMS_TILE);
  hipLaunchKernelGGL(ripe_nms3_kernel, dim3(tx * ty, batch), dim3(256), 0, s, heat, key, thr, H, W, tx);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_map_max(const float* heat, float* partial, float* mapmax, int batch, int n, hipStream_t s) {
  if (batch <= 0 || n <= 0) return 0;
  const int nblk = ripe_max_blocks(n);
  hipLaunchKernelGGL(ripe_max_partial_kernel, dim3(nblk, batch), dim3(256), 0, s, heat, partial, n);
  DIM_LAUNCH_CHECK();
  hipLaunchKernelGGL(ripe_max_finish_kernel, dim3(batch), dim3(256), 0, s, (const float*)partial, nblk, mapmax);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_hypercolumn(const RipeLevels& lv, const float* kpts, const int* n_kpts, float* rows, int capacity, int batch, int H, int W, hipStream_t s) {
  DIM_REQUIRE(H >= 2 && W >= 2, "ripe hypercolumn: image %d x %d (the grid divides by size - 1)", H, W);
  DIM_REQUIRE(batch <= 65535, "ripe hypercolumn: batch %d", batch);
  if (batch <= 0 || capacity <= 0) return 0;
  hipLaunchKernelGGL(ripe_hyper_kernel, dim3(capacity, batch), dim3(256), 0, s, lv, kpts, n_kpts, rows, capacity, H, W);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ripe_desc_finish(const float* lin, const float* raw_scores, const float* mapmax, const int* n_kpts, float* desc, float* scores, int capacity, int batch,
                            hipStream_t s) {
  if (batch <= 0 || capacity <= 0) return 0;
  hipLaunchKernelGGL(ripe_desc_finish_kernel, dim3(cdiv(capacity, 4), batch), dim3(256), 0, s, lin, raw_scores, mapmax, n_kpts, desc, scores, capacity);
  DIM_LAUNCH_CHECK();
  return 0;
}
