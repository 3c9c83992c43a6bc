// LighterGlue (LightGlue at descriptor_dim 96, one head of 96, hidden width 192; reference
// thirdparty/accelerated_features/modules/lighterglue.py:12-27) — the non-GEMM kernels of lg_kernels.hip that index by the width,
// at that width.  Same contracts, same gating (done / n_cur), same guard sites.  One wave per row: a 96-wide row is 24 lanes x float4,
// a 192-wide hidden row 48 lanes x float4; the idle lanes contribute zeros to the wave reductions.
#include <math.h>

#include "lg_kernels.h"

namespace {
constexpr int D = 96, HF = 48, HID = 192;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float4 ld4_if(const float* p, int lane, int width) {
  return lane * 4 < width ? *(const float4*)(p + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// init (lg_init_kernel): keypoint normalisation (LGN:25-34, size used as given), positional encoding over 48 frequencies (LGN:57-70:
// Wr is (head_dim / 2, 2)), index / prune / done bookkeeping.  The descriptors come from input_proj (64 -> 96), never copied.
// grid: (ceil(nmax / 4), items), block 256 = 4 points x 64 lanes (48 frequencies).
__global__ __launch_bounds__(256) void lgl_init_kernel(LgState st, const float* __restrict__ kpts_tab, const int* __restrict__ n_tab,
                                                       const float* __restrict__ size_tab, const int* __restrict__ pair_idx, int cap,
                                                       const float* __restrict__ Wr) {
  const int item = blockIdx.y;
  const int img = pair_idx ? pair_idx[item] : item;
  const int n = min(min(n_tab[img], st.nmax), cap);
  const int j = threadIdx.x & 63, pt = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st.n_cur[item] = n; st.n_new[item] = n; st.n_orig[item] = n;
    if ((item & 1) == 0) {
      const int img1 = pair_idx ? pair_idx[item + 1] : item + 1;
      const int n1 = min(min(n_tab[img1], st.nmax), cap);
      st.done[item >> 1] = (n == 0 || n1 == 0) ? -1 : 0;  // LGN:491-492 at i = 0 -> stop = 1
      st.cnt_lt[item >> 1] = 0;
    }
  }
  if (pt >= st.nmax) return;
  const size_t row = (size_t)item * st.nmax + pt;
  if (j == 0) { st.ind[row] = pt; st.prune[row] = 1; }
  if (pt >= n || j >= HF) return;
  const float sx = size_tab[img * 2], sy = size_tab[img * 2 + 1];
  const float scale = fmaxf(sx, sy) / 2.0f;
  const float kx = (kpts_tab[((size_t)img * cap + pt) * 2] - sx / 2.0f) / scale;
  const float ky = (kpts_tab[((size_t)img * cap + pt) * 2 + 1] - sy / 2.0f) / scale;
  const float pr = kx * Wr[j * 2] + ky * Wr[j * 2 + 1];
  st.enc[row * D + j] = cosf(pr);
  st.enc[row * D + HF + j] = sinf(pr);
}

// LayerNorm(192, eps 1e-5, affine) + exact-erf GELU in place on hid (LGN:141-142); one wave per row.
__global__ __launch_bounds__(256) void lgl_ln_gelu_kernel(LgState st, const float* __restrict__ gamma, const float* __restrict__ beta) {
  const int item = blockIdx.y;
  if (st.done[item >> 1] != 0) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= st.n_cur[item]) return;
  float* p = st.hid + ((size_t)item * st.nmax + row) * HID;
  const bool on = lane * 4 < HID;
  const float4 a = ld4_if(p, lane, HID);
  float x[4] = {a.x, a.y, a.z, a.w};
  const float mean = wave_sum((x[0] + x[1]) + (x[2] + x[3])) / (float)HID;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { const float d = on ? x[i] - mean : 0.0f; sq += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)HID + 1e-5f);
  if (!on) return;
  const float4 g = *(const float4*)(gamma + lane * 4), b = *(const float4*)(beta + lane * 4);
  const float gm[4] = {g.x, g.y, g.z, g.w}, bt[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float y = (x[i] - mean) * rstd * gm[i] + bt[i];
    x[i] = 0.5f * y * (1.0f + erf_1ulp(y * 0.70710678118654752440f));
  }
  *(float4*)(p + lane * 4) = make_float4(x[0], x[1], x[2], x[3]);
  sat_report(st.sat_ffn, sat_track(sat_track(0.0f, x[0], x[1]), x[2], x[3]));
}

// token confidence (LGN:73-83) and matchability (LGN:277-278) per live point + the per-pair count of points with confidence < thr
// (LGN:600-603): lg_confidence_kernel's shape — CONF_ROWS points per wave, one atomic per workgroup.
constexpr int CONF_ROWS = 8;
__global__ __launch_bounds__(256) void lgl_confidence_kernel(LgState st, const float* __restrict__ w_tok, const float* __restrict__ b_tok,
                                                             const float* __restrict__ w_match, const float* __restrict__ b_match, float thr,
                                                             int use_token) {
  __shared__ int blk_cnt[4];
  const int item = blockIdx.y;
  if (st.done[item >> 1] != 0) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + wv) * CONF_ROWS, n = st.n_cur[item];
  if (blockIdx.x * 4 * CONF_ROWS >= n) return;   // (block-uniform)
  const float4 wm = ld4_if(w_match, lane, D);
  float4 wt = make_float4(0.f, 0.f, 0.f, 0.f);
  if (use_token) wt = ld4_if(w_tok, lane, D);
  float4 d[CONF_ROWS];
#pragma unroll
  for (int i = 0; i < CONF_ROWS; ++i) d[i] = ld4_if(st.desc + ((size_t)item * st.nmax + min(row0 + i, n - 1)) * D, lane, D);
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < CONF_ROWS; ++i) {
    const int row = row0 + i;
    if (row >= n) break;   // (wave-uniform)
    const size_t r = (size_t)item * st.nmax + row;
    const float zm = wave_sum(dot4(d[i], wm)) + b_match[0];
    float cf = 0.0f;
    if (use_token) cf = sigmoidf_(wave_sum(dot4(d[i], wt)) + b_tok[0]);
    if (lane == 0) { st.mtch[r] = sigmoidf_(zm); st.conf[r] = cf; }
    cnt += (use_token && cf < thr) ? 1 : 0;
  }
  if (lane == 0) blk_cnt[wv] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = (blk_cnt[0] + blk_cnt[1]) + (blk_cnt[2] + blk_cnt[3]);
    if (c) atomicAdd(&st.cnt_lt[item >> 1], c);
  }
}

// pruning, the two passes that move rows (lg_prune_gather_kernel / lg_prune_copyback_kernel): kept rows into scratch, counters bumped (LGN:509,516) ...
__global__ __launch_bounds__(256) void lgl_prune_gather_kernel(LgState st, int pruning_min) {
  const int item = blockIdx.y;
  if (st.done[item >> 1] != 0) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (st.n_cur[item] <= pruning_min || row >= st.n_cur[item]) return;
  const size_t base = (size_t)item * st.nmax;
  const bool identity = st.n_new[item] == st.n_cur[item];   // nothing pruned on this side: only the counters move
  const int d = st.dest[base + row];
  if (d < 0) return;
  if (!identity) {
    if (lane * 4 < D) *(float4*)(st.tdesc + (base + d) * D + lane * 4) = *(const float4*)(st.desc + (base + row) * D + lane * 4);
    st.tenc[(base + d) * D + lane] = st.enc[(base + row) * D + lane];
    if (lane + 64 < D) st.tenc[(base + d) * D + 64 + lane] = st.enc[(base + row) * D + 64 + lane];
  }
  if (lane == 0) {
    const int orig = st.ind[base + row];
    if (!identity) st.tind[base + d] = orig;
    st.prune[base + orig] += 1;
  }
}
// ... and back
__global__ __launch_bounds__(256) void lgl_prune_copyback_kernel(LgState st, int pruning_min) {
  const int item = blockIdx.y;
  if (st.done[item >> 1] != 0) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (st.n_cur[item] <= pruning_min || row >= st.n_new[item] || st.n_new[item] == st.n_cur[item]) return;
  const size_t r = (size_t)item * st.nmax + row;
  if (lane * 4 < D) *(float4*)(st.desc + r * D + lane * 4) = *(const float4*)(st.tdesc + r * D + lane * 4);
  st.enc[r * D + lane] = st.tenc[r * D + lane];
  if (lane + 64 < D) st.enc[r * D + 64 + lane] = st.tenc[r * D + 64 + lane];
  if (lane == 0) st.ind[r] = st.tind[r];
}

// mdesc = final_proj(desc) / d^0.25 (LGN:268-270) for the pairs with done == tag: a true division by the fp32 value of 96^0.25, as the reference's
// tensor / scalar.  The similarity GEMM splits md, so this is where its range is guarded.
__global__ __launch_bounds__(256) void lgl_scale_md_kernel(LgState st, int tag, unsigned* sat) {
  const int item = blockIdx.y;
  if (st.done[item >> 1] != tag) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= st.n_cur[item] || lane * 4 >= D) return;
  const float c = 3.1301691601465746f;   // 96^0.25
  float4* p = (float4*)(st.md + ((size_t)item * st.nmax + row) * D + lane * 4);
  float4 v = *p;
  v.x /= c; v.y /= c; v.z /= c; v.w /= c;
  *p = v;
  sat_report(sat, sat_track(sat_track(0.0f, v.x, v.y), v.z, v.w));
}
}  // namespace

int launch_lgl_init(const LgState& st, const float* kpts_tab, const int* n_tab, const float* size_tab, const int* pair_idx, int cap, const float* Wr, hipStream_t s) {
  hipLaunchKernelGGL(lgl_init_kernel, dim3(cdiv(st.nmax, 4), st.n_items), dim3(256), 0, s, st, kpts_tab, n_tab, size_tab, pair_idx, cap, Wr);
  DIM_LAUNCH_CHECK();
  return 0;
}
int launch_lgl_ln_gelu(const LgState& st, const float* gamma, const float* beta, hipStream_t s) {
  hipLaunchKernelGGL(lgl_ln_gelu_kernel, dim3(cdiv(st.nsel, 4), st.n_items), dim3(256), 0, s, st, gamma, beta);
  DIM_LAUNCH_CHECK();
  return 0;
}
int launch_lgl_confidence(const LgState& st, const float* w_tok, const float* b_tok, const float* w_match, const float* b_match, float thr, int use_token, hipStream_t s) {
  hipLaunchKernelGGL(lgl_confidence_kernel, dim3(cdiv(st.nsel, 4 * CONF_ROWS), st.n_items), dim3(256), 0, s, st, w_tok, b_tok, w_match, b_match, thr, use_token);
  DIM_LAUNCH_CHECK();
  return 0;
}
int launch_lgl_prune_move(const LgState& st, int pruning_min, hipStream_t s) {
  hipLaunchKernelGGL(lgl_prune_gather_kernel, dim3(cdiv(st.nsel, 4), st.n_items), dim3(256), 0, s, st, pruning_min);
  hipLaunchKernelGGL(lgl_prune_copyback_kernel, dim3(cdiv(st.nsel, 4), st.n_items), dim3(256), 0, s, st, pruning_min);
  DIM_LAUNCH_CHECK();
  return 0;
}
int launch_lgl_scale_md(const LgState& st, int tag, unsigned* sat, hipStream_t s) {
  hipLaunchKernelGGL(lgl_scale_md_kernel, dim3(cdiv(st.nsel, 4), st.n_items), dim3(256), 0, s, st, tag, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}
