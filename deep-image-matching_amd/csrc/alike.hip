// ALIKE (thirdparty/alike/{alnet,alike,soft_detect}.py) kernels for gfx950: the score map WITHOUT the descriptor map (single-head models: the
// score row of convhead2 is applied to the three low-resolution groups before they are up-sampled), and the sparse descriptor head (convhead2
// only at the four pixels around a keypoint).  The dim-channel maps x1234 / descriptor_map (alnet.py:173-180) are never stored.
// The encoder / aggregation convolutions are nhwc_conv.hip's kernel; the head products are the library's GEMMs.
// Every reduction has a fixed order; no floating-point atomics.
#include "alike_kernels.h"

namespace {

// ---------------------------------------------------------------------------
// bilinear up-sampling with align_corners=True (alnet.py:136-147) of channel `ch` of a low-resolution map [Hl][Wl][stride] at pixel (y, x)
// of the padded frame: source coordinate = index * (in - 1) / (out - 1), second tap clamped at the edge
struct AkTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ AkTap ak_tap(int idx, int in, int out) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const float f = scale * (float)idx;
  AkTap t;
  t.i0 = (int)f;
  if (t.i0 > in - 1) t.i0 = in - 1;
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = f - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}
__device__ __forceinline__ float ak_interp(const float* __restrict__ m, int Wl, int stride, int ch, const AkTap& ty, const AkTap& tx) {
  const float v00 = m[((size_t)ty.i0 * Wl + tx.i0) * stride + ch], v01 = m[((size_t)ty.i0 * Wl + tx.i1) * stride + ch];
  const float v10 = m[((size_t)ty.i1 * Wl + tx.i0) * stride + ch], v11 = m[((size_t)ty.i1 * Wl + tx.i1) * stride + ch];
  return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

__global__ __launch_bounds__(256) void ak_project_kernel(const float* __restrict__ f, int fq, int q, const float* __restrict__ ws, float* __restrict__ out, int n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float* v = f + (size_t)p * fq;
  float s = 0.f;
  for (int c = 0; c < q; ++c) s = fmaf(ws[c], v[c], s);
  out[p] = s;
}

// one thread per pixel of the cropped map; conv1 (c1 -> q, ReLU) and its contraction with w_s[0:q] per pixel, weights in LDS
template <int C1P>
__global__ __launch_bounds__(256) void ak_score_kernel(const AkFeat F, const float* __restrict__ ws, const float* __restrict__ q2, const float* __restrict__ q3,
                                                       const float* __restrict__ q4, float* __restrict__ score, int H, int W) {
  __shared__ float w1s[32 * 32], wss[32];
  for (int t = threadIdx.x; t < C1P * F.q; t += 256) w1s[t] = F.w1[t];
  if (threadIdx.x < F.q) wss[threadIdx.x] = ws[threadIdx.x];
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= H * W) return;
  const int y = p / W, x = p % W;
  const int Hp = F.Hp, Wp = F.Wp;
  const float* xv = F.x1 + (((size_t)b * Hp + y) * Wp + x) * F.c1p;
  float xin[C1P];
#pragma unroll
  for (int c = 0; c < C1P; ++c) xin[c] = xv[c];
  float s = 0.f;
  for (int j = 0; j < F.q; ++j) {
    float t = 0.f;
#pragma unroll
    for (int c = 0; c < C1P; ++c) t = fmaf(w1s[c * F.q + j], xin[c], t);
    s = fmaf(wss[j], fmaxf(t, 0.f), s);
  }
  const int H2 = Hp / 2, W2 = Wp / 2, H8 = Hp / 8, W8 = Wp / 8, H32 = Hp / 32, W32 = Wp / 32;
  s += ak_interp(q2 + (size_t)b * H2 * W2, W2, 1, 0, ak_tap(y, H2, Hp), ak_tap(x, W2, Wp));
  s += ak_interp(q3 + (size_t)b * H8 * W8, W8, 1, 0, ak_tap(y, H8, Hp), ak_tap(x, W8, Wp));
  s += ak_interp(q4 + (size_t)b * H32 * W32, W32, 1, 0, ak_tap(y, H32, Hp), ak_tap(x, W32, Wp));
  score[(size_t)b * H * W + p] = 1.0f / (1.0f + expf(-s));
}

// one thread per (row, channel j < q): the four groups' channel j of the row's pixel
__global__ __launch_bounds__(256) void ak_rows_kernel(const AkFeat F, const float* __restrict__ kpts_norm, const int* __restrict__ n_kpts, int capacity, int y0,
                                                      int n_rows, float* __restrict__ X, int ldx, long long strideX, int H, int W, unsigned* sat) {
  const int b = blockIdx.y;
  const int rows = kpts_norm != nullptr ? 4 * n_kpts[b] : n_rows;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(item / F.q), j = (int)(item % F.q);
  if (row >= rows) return;
  int x, y;
  if (kpts_norm != nullptr) {
    const size_t k = (size_t)b * capacity + (row >> 2);
    const float ix = ((kpts_norm[k * 2] + 1.f) / 2.f) * (float)(W - 1), iy = ((kpts_norm[k * 2 + 1] + 1.f) / 2.f) * (float)(H - 1);
    x = (int)floorf(ix) + (row & 1); y = (int)floorf(iy) + ((row >> 1) & 1);
  } else {
    y = y0 + row / W; x = row % W;
  }
  float* dst = X + (size_t)b * strideX + (size_t)row * ldx;
  const int q = F.q;
  if (x < 0 || x >= W || y < 0 || y >= H) {   // grid_sample's zero padding outside the cropped map
    dst[j] = 0.f; dst[q + j] = 0.f; dst[2 * q + j] = 0.f; dst[3 * q + j] = 0.f;
    return;
  }
  const int Hp = F.Hp, Wp = F.Wp;
  const float* xv = F.x1 + (((size_t)b * Hp + y) * Wp + x) * F.c1p;
  float t = 0.f;
  for (int c = 0; c < F.c1p; ++c) t = fmaf(F.w1[c * q + j], xv[c], t);
  const int H2 = Hp / 2, W2 = Wp / 2, H8 = Hp / 8, W8 = Wp / 8, H32 = Hp / 32, W32 = Wp / 32;
  const float g0 = fmaxf(t, 0.f);
  const float g1 = ak_interp(F.f2 + (size_t)b * H2 * W2 * F.fq, W2, F.fq, j, ak_tap(y, H2, Hp), ak_tap(x, W2, Wp));
  const float g2 = ak_interp(F.f3 + (size_t)b * H8 * W8 * F.fq, W8, F.fq, j, ak_tap(y, H8, Hp), ak_tap(x, W8, Wp));
  const float g3 = ak_interp(F.f4 + (size_t)b * H32 * W32 * F.fq, W32, F.fq, j, ak_tap(y, H32, Hp), ak_tap(x, W32, Wp));
  dst[j] = g0; dst[q + j] = g1; dst[2 * q + j] = g2; dst[3 * q + j] = g3;
  sat_report(sat, fmaxf(fmaxf(g0, g1), fmaxf(g2, g3)));   // inputs of the split-precision head products
}

__global__ __launch_bounds__(256) void ak_contract_kernel(const float* __restrict__ hid, int ldh, long long strideH, const float* __restrict__ ws, int dim,
                                                          float* __restrict__ score, int y0, int n_rows, int H, int W) {
  const int r = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (r >= n_rows) return;
  const float* v = hid + (size_t)b * strideH + (size_t)r * ldh;
  float s = 0.f;
  for (int c = 0; c < dim; ++c) s = fmaf(ws[c], v[c], s);
  score[(size_t)b * H * W + (size_t)y0 * W + r] = 1.0f / (1.0f + expf(-s));
}

__global__ __launch_bounds__(256) void ak_border_kernel(float* __restrict__ nms, int H, int W) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= H * W) return;
  const int y = p / W, x = p % W;
  if (y < 3 || x < 3 || y >= H - 2 || x >= W - 2) nms[(size_t)b * H * W + p] = 0.f;
}

// one wave per keypoint, lane -> channels lane, lane + 64; the sums run through wave_sum's fixed butterfly
__global__ __launch_bounds__(256) void ak_desc_blend_kernel(const float* __restrict__ D, int ldd, long long strideD, const float* __restrict__ kpts_norm, const int* __restrict__ n_kpts,
                                                            float* __restrict__ desc, int dim, int stride, int capacity, int H, int W) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (k >= n_kpts[b]) return;
  const size_t kk = (size_t)b * capacity + k;
  const float ix = ((kpts_norm[kk * 2] + 1.f) / 2.f) * (float)(W - 1), iy = ((kpts_norm[kk * 2 + 1] + 1.f) / 2.f) * (float)(H - 1);
  const float fx = floorf(ix), fy = floorf(iy);
  const float wts[4] = {(fx + 1.f - ix) * (fy + 1.f - iy), (ix - fx) * (fy + 1.f - iy), (fx + 1.f - ix) * (iy - fy), (ix - fx) * (iy - fy)};
  const float* rows = D + (size_t)b * strideD + (size_t)k * 4 * ldd;
  const int c0 = lane, c1 = lane + 64;
  float o0 = 0.f, o1 = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float a0 = c0 < dim ? rows[(size_t)c * ldd + c0] : 0.f, a1 = c1 < dim ? rows[(size_t)c * ldd + c1] : 0.f;
    const float n = fmaxf(sqrtf(wave_sum(a0 * a0 + a1 * a1)), 1e-12f);   // F.normalize of the dense map's pixel (alike.py:125)
    o0 += (a0 / n) * wts[c]; o1 += (a1 / n) * wts[c];
  }
  const float n = fmaxf(sqrtf(wave_sum(o0 * o0 + o1 * o1)), 1e-12f);     // soft_detect.py:68
  float* out = desc + kk * stride;
  if (c0 < stride) out[c0] = c0 < dim ? o0 / n : 0.f;
  if (c1 < stride) out[c1] = c1 < dim ? o1 / n : 0.f;
}

}  // namespace

int launch_ak_project(const float* f, int fq, int q, const float* ws, float* out, int n_pixels, hipStream_t s) {
  hipLaunchKernelGGL(ak_project_kernel, dim3(cdiv(n_pixels, 256)), dim3(256), 0, s, f, fq, q, ws, out, n_pixels);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ak_score(const AkFeat& F, const float* ws, const float* q2, const float* q3, const float* q4, float* score, int batch, int H, int W, hipStream_t s) {
  DIM_REQUIRE((F.c1p == 16 || F.c1p == 32) && F.q <= 32, "ak_score: c1 %d / q %d", F.c1p, F.q);
  if (F.c1p == 16) hipLaunchKernelGGL(HIP_KERNEL_NAME(ak_score_kernel<16>), dim3(cdiv(H * W, 256), batch), dim3(256), 0, s, F, ws, q2, q3, q4, score, H, W);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(ak_score_kernel<32>), dim3(cdiv(H * W, 256), batch), dim3(256), 0, s, F, ws, q2, q3, q4, score, H, W);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ak_rows(const AkFeat& F, const float* kpts_norm, const int* n_kpts, int capacity, int y0, int n_rows, float* X, int ldx, long long strideX,
                   int batch, int H, int W, unsigned* sat, hipStream_t s) {
  const long long items = (long long)(kpts_norm != nullptr ? 4 * capacity : n_rows) * F.q;
  DIM_REQUIRE(items > 0 && 4 * F.q <= ldx, "ak_rows: %lld items, row length %d", items, ldx);
  hipLaunchKernelGGL(ak_rows_kernel, dim3((unsigned)((items + 255) / 256), batch), dim3(256), 0, s, F, kpts_norm, n_kpts, capacity, y0, n_rows, X, ldx, strideX, H, W, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ak_contract(const float* hid, int ldh, long long strideH, const float* ws, int dim, float* score, int y0, int n_rows, int batch, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(ak_contract_kernel, dim3(cdiv(n_rows, 256), batch), dim3(256), 0, s, hid, ldh, strideH, ws, dim, score, y0, n_rows, H, W);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ak_border(float* nms, int batch, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(ak_border_kernel, dim3(cdiv(H * W, 256), batch), dim3(256), 0, s, nms, H, W);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_ak_desc_blend(const float* D, int ldd, long long strideD, const float* kpts_norm, const int* n_kpts, float* desc, int dim, int stride, int capacity, int batch,
                         int H, int W, hipStream_t s) {
  DIM_REQUIRE(dim <= 128 && stride <= 128 && stride >= dim, "ak_desc_blend: dim %d / stride %d", dim, stride);
  hipLaunchKernelGGL(ak_desc_blend_kernel, dim3(cdiv(capacity, 4), batch), dim3(256), 0, s, D, ldd, strideD, kpts_norm, n_kpts, desc, dim, stride, capacity, H, W);
  DIM_LAUNCH_CHECK();
  return 0;
}
