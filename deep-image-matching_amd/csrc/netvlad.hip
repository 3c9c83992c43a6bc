// NetVLAD global descriptor (thirdparty/hloc/extractors/netvlad.py = NV): the kernels around the VGG16 convolutions.
//
//   nv_conv1_kernel        conv1_1 with the input normalisation in its operand load (3 -> 64, fp32 FMAs: 27 products per output)
//   nv_maxpool_kernel      2 x 2 max-pool, floor semantics
//   nv_head_block_kernel   per block of 128 locations: L2 normalisation over the 512 channels, the 512 -> K scores, the softmax over K and the
//                          block's partial aggregate sum_n s[n][k] x^[n][d] on the matrix cores (v_mfma_f32_32x32x2_f32: fp32 operands, so the
//                          normalised map and the scores are used as they are) — neither the normalised map nor the scores reach HBM
//   nv_head_finish_kernel  fixed-order sum of the blocks' partials, the centre term, intra-normalisation, flatten to d K + k, global L2
//   nv_whiten_*            y = W v + b with W [out][512 K] streamed ONCE for up to 16 images, K split over workgroups, fixed-order reduction, L2
//
// Every sum has a fixed order (no floating-point atomics): a result depends on the image alone, not on the batch around it.
#include <math.h>

#include "netvlad_kernels.h"

namespace {
constexpr int LB = 16;                      // locations per sub-block (LDS image of the normalised map: 16 x 544 fp32 = 34 KB)
constexpr int XS = NV_D + 32;               // row stride of that image: rows 2 s and 2 s + 1 (the two lane halves of an MFMA operand read) lie 32 banks apart
constexpr int SUBS = NV_WG_LOCS / LB;       // sub-blocks one workgroup walks through, accumulators kept in registers

__device__ __forceinline__ float clamp_norm(float x, float mean) { return fminf(fmaxf(255.0f * x, 0.0f), 255.0f) - mean; }

// 64 pixels x 4 groups of 16 output channels per workgroup
__global__ __launch_bounds__(256) void nv_conv1_kernel(const float* __restrict__ image, const float* __restrict__ mean3, const float* __restrict__ w,
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
    const float m = mean3[ci];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int gy = y + dy - 1, gx = x + dx - 1;
        float v = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
          const float px = img[((size_t)gy * W + gx) * 3 + ci];
          bad |= !(px == px);   // the clamp drops a NaN (it reads as 0 - mean): reported where a guard counter is given (include/dim_hip.h)
          v = clamp_norm(px, m);
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

__global__ __launch_bounds__(256) void nv_maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C4, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // i = ((image * Ho + y) * Wo + x) * C4 + channel quad
  if (i >= n) return;
  const int Ho = H >> 1, Wo = W >> 1;
  const size_t c = i % C4, px = i / C4, x = px % Wo, r = px / Wo, y = r % Ho, b = r / Ho;
  const float4* s = (const float4*)in + ((b * H + 2 * y) * W + 2 * x) * C4 + c;
  const float4 a = s[0], bq = s[C4], cq = s[(size_t)W * C4], d = s[(size_t)W * C4 + C4];
  float4 o;
  o.x = fmaxf(fmaxf(a.x, bq.x), fmaxf(cq.x, d.x)); o.y = fmaxf(fmaxf(a.y, bq.y), fmaxf(cq.y, d.y));
  o.z = fmaxf(fmaxf(a.z, bq.z), fmaxf(cq.z, d.z)); o.w = fmaxf(fmaxf(a.w, bq.w), fmaxf(cq.w, d.w));
  ((float4*)out)[i] = o;
}

// ---- head, stage 1 -------------------------------------------------------------------------------------------------------------------
// Workgroup (blk, b) = locations blk * 128 .. + 127 of image b in sub-blocks of 16; 4 waves.  Per sub-block:
//   1. wave w loads and normalises locations 4 w .. 4 w + 3 (F.normalize, NV:138: x / max(||x||, 1e-12)) into xs[16][512];
//   2. wave w, lane k: the scores of those four locations against cluster k (an fmaf chain over d, NV:30), the softmax over the wave's lanes
//      (NV:31) into ss[16][64]; locations past n and clusters past K hold zeros;
//   3. the aggregate as M = k (2 tiles), N = d (16 tiles), K-dim = location: wave w owns d tiles 4 w .. 4 w + 3 of both k tiles
//      = 8 accumulators; one 32x32x2 MFMA takes two locations: A[i = k][location] = ss, B[location][j = d] = xs.
// Output: part[(b * nblk + blk)][k][d] (coalesced over d) followed by the block's sum_n s[n][k] (64 floats).
__global__ __launch_bounds__(256) void nv_head_block_kernel(const float* __restrict__ x, int n, int K, const float* __restrict__ score_dk,
                                                            float* __restrict__ part, int nblk) {
  __shared__ float xs[LB * XS];
  __shared__ float ss[LB * NV_KMAX];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lx = lane & 31, half = lane >> 5;
  const int blk = blockIdx.x, b = blockIdx.y;
  const float* xb = x + (size_t)b * n * NV_D;
  const int nkt = K > 32 ? 2 : 1;
  f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  float colsum = 0.0f;   // threads 0 .. 63: sum_n s[n][t] of this workgroup's locations

  for (int sub = 0; sub < SUBS; ++sub) {
    const int n0 = (blk * SUBS + sub) * LB;
    if (n0 >= n) break;   // uniform
    __syncthreads();      // every wave is done with the previous sub-block's xs / ss
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int l = 4 * wv + j, loc = n0 + l;
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
      if (loc < n) {
        v0 = *(const float4*)(xb + (size_t)loc * NV_D + lane * 4);
        v1 = *(const float4*)(xb + (size_t)loc * NV_D + 256 + lane * 4);
      }
      float q = v0.x * v0.x;
      q = fmaf(v0.y, v0.y, q); q = fmaf(v0.z, v0.z, q); q = fmaf(v0.w, v0.w, q);
      q = fmaf(v1.x, v1.x, q); q = fmaf(v1.y, v1.y, q); q = fmaf(v1.z, v1.z, q); q = fmaf(v1.w, v1.w, q);
      const float den = fmaxf(sqrtf(wave_sum(q)), 1e-12f);
      v0.x /= den; v0.y /= den; v0.z /= den; v0.w /= den;
      v1.x /= den; v1.y /= den; v1.z /= den; v1.w /= den;
      *(float4*)&xs[l * XS + lane * 4] = v0;
      *(float4*)&xs[l * XS + 256 + lane * 4] = v1;
    }
    __syncthreads();
    float sc[4] = {0.f, 0.f, 0.f, 0.f};
    if (lane < K) {
      for (int d = 0; d < NV_D; ++d) {
        const float w = score_dk[(size_t)d * K + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j] = fmaf(xs[(4 * wv + j) * XS + d], w, sc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = lane < K ? sc[j] : -INFINITY;
      const float m = wave_max(v);
      const float e = lane < K ? expf(v - m) : 0.0f;
      const float tot = wave_sum(e);
      ss[(4 * wv + j) * NV_KMAX + lane] = (n0 + 4 * wv + j < n) ? e / tot : 0.0f;
    }
    __syncthreads();
    if (t < NV_KMAX) {
#pragma unroll
      for (int l = 0; l < LB; ++l) colsum += ss[l * NV_KMAX + t];
    }
#pragma unroll
    for (int step = 0; step < LB / 2; ++step) {
      const int row = 2 * step + half;
      float a[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) a[kt] = ss[row * NV_KMAX + kt * 32 + lx];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const float bv = xs[row * XS + (4 * wv + dt) * 32 + lx];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          if (kt < nkt) acc[kt][dt] = mfma32(a[kt], bv, acc[kt][dt]);
      }
    }
  }

  float* pb = part + ((size_t)b * nblk + blk) * nv_head_part_stride(K);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = kt * 32 + mfma_row(r, half), d = (4 * wv + dt) * 32 + lx;
        if (k < K) pb[(size_t)k * NV_D + d] = acc[kt][dt][r];
      }
  if (t < NV_KMAX) pb[(size_t)K * NV_D + t] = colsum;
}

// sum over the 256 threads of a workgroup in a fixed order; red: 4 floats of LDS
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();   // the previous call's readers are done with red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- head, stage 2: one workgroup per image, thread t owns d = t and t + 256 ---------------------------------------------------------------
// V[d][k] = sum_blk P[blk][k][d] - c[d][k] sum_blk S[blk][k]  (NV:32-33: sum_n s (x - c)), column k divided by max(||V[:, k]||, 1e-12) (NV:36),
// stored at d K + k (NV:37), then everything divided by max(||vlad||, 1e-12) (NV:38) — each thread rescales the elements it wrote itself.
__global__ __launch_bounds__(256) void nv_head_finish_kernel(const float* __restrict__ part, int nblk, int K, const float* __restrict__ centers_kd,
                                                             float* __restrict__ vlad) {
  __shared__ float S[NV_KMAX];
  __shared__ float red[4];
  const int t = threadIdx.x, b = blockIdx.x;
  const size_t ps = nv_head_part_stride(K);
  const float* pb = part + (size_t)b * nblk * ps;
  float* o = vlad + (size_t)b * K * NV_D;
  if (t < K) {
    float s = 0.0f;
    for (int i = 0; i < nblk; ++i) s += pb[i * ps + (size_t)K * NV_D + t];
    S[t] = s;
  }
  __syncthreads();
  float total = 0.0f;
  for (int k = 0; k < K; ++k) {
    float v0 = 0.0f, v1 = 0.0f;
    for (int i = 0; i < nblk; ++i) {
      v0 += pb[i * ps + (size_t)k * NV_D + t];
      v1 += pb[i * ps + (size_t)k * NV_D + 256 + t];
    }
    v0 = fmaf(-centers_kd[(size_t)k * NV_D + t], S[k], v0);
    v1 = fmaf(-centers_kd[(size_t)k * NV_D + 256 + t], S[k], v1);
    const float den = fmaxf(sqrtf(block_sum256(fmaf(v1, v1, v0 * v0), red)), 1e-12f);
    v0 /= den; v1 /= den;
    total += block_sum256(fmaf(v1, v1, v0 * v0), red);
    o[(size_t)t * K + k] = v0;
    o[(size_t)(t + 256) * K + k] = v1;
  }
  const float den = fmaxf(sqrtf(total), 1e-12f);
  for (int k = 0; k < K; ++k) {
    o[(size_t)t * K + k] /= den;
    o[(size_t)(t + 256) * K + k] /= den;
  }
}

// ---- whitening ---------------------------------------------------------------------------------------------------------------------
// Workgroup (og, ks): output rows 16 og .. 16 og + 15 over k in [ks KC, (ks + 1) KC); wave w owns rows 16 og + 4 w .. + 3 and walks the whole k range
// with its 64 lanes: every lane streams float4s of the four W rows and multiplies each into the NB images' vectors (fmaf chains), then the 64 lanes'
// sums are added by a shuffle tree.  The four waves read the same slices of the vectors (from L1 / L2: NB x 16 KB per workgroup against 256 KB of W).
// One image's chain does not involve the others: its result is the same for every NB and every batch.  part[ks][batch][out].
constexpr int WH_ROWS = 16;
template <int NB>
__global__ __launch_bounds__(256) void nv_whiten_partial_kernel(const float* __restrict__ Wm, const float* __restrict__ v, int batch, int in_dim, int out_dim,
                                                                float* __restrict__ part) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int o0 = blockIdx.x * WH_ROWS + 4 * wv, k0 = blockIdx.y * NV_WHITEN_KC;
  if (o0 >= out_dim) return;   // wave-uniform; no barrier below
  float acc[4][NB];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[r][i] = 0.0f;
  const float* wr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) wr[r] = Wm + (size_t)min(o0 + r, out_dim - 1) * in_dim;
#pragma unroll 1   // left to itself the compiler unrolls all 16 steps of the NB = 2 instance and hoists their loads: 256 VGPRs + 146 AGPRs, one wave per SIMD
  for (int it = 0; it < NV_WHITEN_KC / 256; ++it) {
    const int kk = k0 + it * 256 + lane * 4;
    float4 vv[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) vv[i] = *(const float4*)(v + (size_t)min(i, batch - 1) * in_dim + kk);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float4 w4 = *(const float4*)(wr[r] + kk);
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        float a = acc[r][i];
        a = fmaf(w4.x, vv[i].x, a); a = fmaf(w4.y, vv[i].y, a); a = fmaf(w4.z, vv[i].z, a); a = fmaf(w4.w, vv[i].w, a);
        acc[r][i] = a;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const float s = wave_sum(acc[r][i]);
      if (lane == 0 && i < batch && o0 + r < out_dim) part[((size_t)blockIdx.y * batch + i) * out_dim + o0 + r] = s;
    }
}

// one workgroup per image: y[o] = sum_ks part[ks][b][o] + bias[o] in k order, then y / max(||y||, 1e-12)
__global__ __launch_bounds__(256) void nv_whiten_finish_kernel(const float* __restrict__ part, int nks, int batch, int out_dim, const float* __restrict__ bias,
                                                               float* __restrict__ y) {
  __shared__ float red[4];
  const int t = threadIdx.x, b = blockIdx.x;
  float* o = y + (size_t)b * out_dim;
  float q = 0.0f;
  for (int i = t; i < out_dim; i += 256) {
    float s = 0.0f;
    for (int ks = 0; ks < nks; ++ks) s += part[((size_t)ks * batch + b) * out_dim + i];
    s += bias[i];
    o[i] = s;
    q = fmaf(s, s, q);
  }
  const float den = fmaxf(sqrtf(block_sum256(q, red)), 1e-12f);
  for (int i = t; i < out_dim; i += 256) o[i] /= den;
}
}  // namespace

int launch_nv_conv1(const float* image, const float* mean3, const float* w_27x64, const float* bias, float* out, int batch, int H, int W, unsigned* sat,
                    hipStream_t s) {
  DIM_REQUIRE((long long)H * W <= 0x7fffffffLL / 64, "netvlad conv1: image %d x %d too large", H, W);
  if (batch <= 0 || H <= 0 || W <= 0) return 0;
  hipLaunchKernelGGL(nv_conv1_kernel, dim3(cdiv(H * W, 64), batch), dim3(256), 0, s, image, mean3, w_27x64, bias, out, H, W, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_nv_maxpool(const float* in, float* out, int batch, int H, int W, int C, hipStream_t s) {
  DIM_REQUIRE(C % 4 == 0, "netvlad maxpool: %d channels (a multiple of 4)", C);
  const size_t n = (size_t)batch * (H / 2) * (W / 2) * (C / 4);
  if (batch <= 0 || n == 0) return 0;
  DIM_REQUIRE((n + 255) / 256 <= 0x7fffffffull, "netvlad maxpool: %zu items exceed one grid", n);
  hipLaunchKernelGGL(nv_maxpool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, H, W, C / 4, n);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_nv_head(const float* x, int batch, int n, int K, const float* score_dk, const float* centers_kd, float* workspace, float* vlad, hipStream_t s) {
  DIM_REQUIRE(K >= 8 && K <= NV_KMAX && K % 8 == 0, "netvlad head: %d clusters (a multiple of 8 up to %d)", K, NV_KMAX);
  DIM_REQUIRE(n >= 1 && (long long)n * NV_D <= 0x7fffffffLL, "netvlad head: %d locations", n);
  if (batch <= 0) return 0;
  const int nblk = nv_head_blocks(n);
  hipLaunchKernelGGL(nv_head_block_kernel, dim3(nblk, batch), dim3(256), 0, s, x, n, K, score_dk, workspace, nblk);
  DIM_LAUNCH_CHECK();
  hipLaunchKernelGGL(nv_head_finish_kernel, dim3(batch), dim3(256), 0, s, (const float*)workspace, nblk, K, centers_kd, vlad);
  DIM_LAUNCH_CHECK();
  return 0;
}

int launch_nv_whiten(const float* v, int batch, int in_dim, const float* W, const float* bias, int out_dim, float* workspace, float* y, hipStream_t s) {
  DIM_REQUIRE(in_dim > 0 && in_dim % NV_WHITEN_KC == 0, "netvlad whitening: in_dim %d must be a multiple of %d", in_dim, NV_WHITEN_KC);
  DIM_REQUIRE(out_dim >= 1 && out_dim <= (1 << 20), "netvlad whitening: out_dim %d", out_dim);
  const int nks = in_dim / NV_WHITEN_KC;
  for (int b0 = 0; b0 < batch; b0 += NV_WHITEN_NB) {   // W once per 16 images
    const int nb = min(batch - b0, NV_WHITEN_NB);
    const float* vb = v + (size_t)b0 * in_dim;
    const dim3 grid(cdiv(out_dim, WH_ROWS), nks);
#define NV_WHITEN(NB) hipLaunchKernelGGL(HIP_KERNEL_NAME(nv_whiten_partial_kernel<NB>), grid, dim3(256), 0, s, W, vb, nb, in_dim, out_dim, workspace)
    if (nb == 1) NV_WHITEN(1);
    else if (nb == 2) NV_WHITEN(2);
    else if (nb <= 4) NV_WHITEN(4);
    else if (nb <= 8) NV_WHITEN(8);
    else NV_WHITEN(16);
#undef NV_WHITEN
    DIM_LAUNCH_CHECK();
    hipLaunchKernelGGL(nv_whiten_finish_kernel, dim3(nb), dim3(256), 0, s, (const float*)workspace, nks, nb, out_dim, bias, y + (size_t)b0 * out_dim);
    DIM_LAUNCH_CHECK();
  }
  return 0;
}
