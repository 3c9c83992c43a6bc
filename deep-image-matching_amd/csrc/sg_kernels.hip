// SuperGlue's own kernels (reference thirdparty/SuperGluePretrainedNetwork/models/superglue.py, SGN): the keypoint encoder (SGN:64-84), the
// log-domain Sinkhorn iterations of the optimal-transport layer (SGN:152-186) and the match selection (SGN:288-305).  The attentional graph
// network between them runs on the LightGlue GEMM / attention kernels (sg_api.hip).
//
// Optimal transport without the coupling matrix.  The reference concatenates the m x n score block with a dustbin row, column and corner that
// all hold the scalar alpha (bin_score) and iterates on that (m+1) x (n+1) matrix.  Here the block stays where the score GEMM wrote it
// (st.sim, row stride nmax) and the dustbin terms are evaluated analytically: a row's log-sum-exp is the block's plus the one term
// alpha + v[n]; the dustbin row's is alpha + LSE(v).  Only u [m+1] and v [n+1] are ever written, and the final Z = S + u + v - norm is formed
// on the fly by the selection.
//
// Reductions are fp32 with the running maximum subtracted, library expf / logf, and a FIXED order that depends on (m, n) of the pair alone:
//   rows:    one wave per row; lane l takes the columns 4 (l + 64 t) .. + 3, t = 0, 1, ..; per chunk of four one rescale of the running sum; the
//            64 (max, sum) partials meet in an xor butterfly; the dustbin term comes last.
//   columns: 16 columns x 32 row groups per workgroup; group g takes the rows g + 32 t in chunks of four; the 32 partials of a column are
//            combined by one thread in the order g = 0 .. 31; the dustbin term comes last.
// No atomics, no dependence on the batch or on the handle's capacity: a pair gives the same bits alone and in a batch.
#include <math.h>

#include "sg_kernels.h"

namespace {

constexpr int ET = 32;   // keypoints per workgroup of the encoder

// One workgroup per (32 keypoints, item).  Thread c owns output channel c of every stage for all 32 keypoints (32 accumulators); the
// activations of a stage sit in LDS as [channel][keypoint], so a stage's inner loop is one coalesced weight load (w[k][c], L1 / L2 resident:
// 428 KB for the whole encoder) and eight broadcast 16-byte LDS reads per 32 FMAs.  fp32 FMA chains in the order bias, k = 0, 1, ...
__global__ __launch_bounds__(256) void sg_encoder_kernel(LgState st, SgEncW w, const float* __restrict__ kpts_tab, const float* __restrict__ desc_tab,
                                                         const float* __restrict__ score_tab, const int* __restrict__ n_tab,
                                                         const float* __restrict__ size_tab, const int* __restrict__ pair_idx, int cap, unsigned* sat) {
  __shared__ float act[2][256][ET];
  const int item = blockIdx.y, t = threadIdx.x;
  const int img = pair_idx ? pair_idx[item] : item;
  const int n = min(min(n_tab[img], st.nmax), cap);
  if (blockIdx.x == 0 && t == 0) {
    st.n_cur[item] = n;
    if (!(item & 1)) {
      const int img1 = pair_idx ? pair_idx[item + 1] : item + 1;
      const int n1 = min(min(n_tab[img1], st.nmax), cap);
      st.done[item >> 1] = (n == 0 || n1 == 0) ? -1 : 0;   // SGN:255-262: every later launch skips the pair
    }
  }
  const int r0 = blockIdx.x * ET;
  if (r0 >= n) return;
  if (t < 3 * ET) {   // [x', y', score] (SGN:64-71, 83-84)
    const int c = t / ET, j = t - c * ET, row = r0 + j;
    float x = 0.0f;
    if (row < n) {
      const float W = size_tab[img * 2], H = size_tab[img * 2 + 1];
      if (c == 2) x = score_tab[(size_t)img * cap + row];
      else x = (kpts_tab[((size_t)img * cap + row) * 2 + c] - (c == 0 ? W : H) / 2.0f) / (fmaxf(W, H) * 0.7f);
    }
    act[0][c][j] = x;
  }
  __syncthreads();
  const int dims[6] = {3, 32, 64, 128, 256, 256};
  int cur = 0;
#pragma unroll 1
  for (int sidx = 0; sidx < 5; ++sidx) {
    const int cin = dims[sidx], cout = dims[sidx + 1];
    if (t < cout) {
      float acc[ET];
      const float b = w.b[sidx][t];
#pragma unroll
      for (int j = 0; j < ET; ++j) acc[j] = b;
      const float* wp = w.w[sidx] + t;
#pragma unroll 2
      for (int k = 0; k < cin; ++k) {
        const float wv = wp[(size_t)k * cout];
        const float4* a4 = (const float4*)&act[cur][k][0];
#pragma unroll
        for (int j = 0; j < ET / 4; ++j) {
          const float4 a = a4[j];
          acc[4 * j] = fmaf(wv, a.x, acc[4 * j]); acc[4 * j + 1] = fmaf(wv, a.y, acc[4 * j + 1]);
          acc[4 * j + 2] = fmaf(wv, a.z, acc[4 * j + 2]); acc[4 * j + 3] = fmaf(wv, a.w, acc[4 * j + 3]);
        }
      }
      if (sidx < 4) {
#pragma unroll
        for (int j = 0; j < ET; ++j) act[cur ^ 1][t][j] = fmaxf(acc[j], 0.0f);
      } else {   // desc = descriptors + encoder (SGN:269-270)
        float vmax = 0.0f;
#pragma unroll
        for (int j = 0; j < ET; ++j) {
          const int row = r0 + j;
          if (row < n) {
            const float y = desc_tab[((size_t)img * cap + row) * 256 + t] + acc[j];
            st.desc[((size_t)item * st.nmax + row) * 256 + t] = y;
            vmax = sat_track(vmax, y, y);
          }
        }
        sat_report(sat, vmax);
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

// (max, sum) of a chunk of four folded into the running pair: one rescale of the sum per chunk.  x may hold -inf (masked), never all four.
__device__ __forceinline__ void lse_fold4(float& mx, float& sm, const float (&x)[4]) {
  const float cm = fmaxf(fmaxf(mx, fmaxf(x[0], x[1])), fmaxf(x[2], x[3]));
  sm = sm * expf(mx - cm) + (((expf(x[0] - cm) + expf(x[1] - cm)) + expf(x[2] - cm)) + expf(x[3] - cm));
  mx = cm;
}
// ... and the closing step: the dustbin term xd joins (M, tot), and the potential log_marginal - (max + log(sum)) is formed in fp64 and rounded
// ONCE.  One log per row / column, so the cost is nothing; the reason is the iteration's neutral direction: (u - c, v + c) leaves Z + u + v
// unchanged, so a bias of the closing step that differs between the row and the column pass is never contracted away but adds up over the
// iterations.  With fp32 logf and three fp32 roundings here the MI355X drifted by 5e-7 per iteration at 1100 x 900 (a uniform shift of u against
// v, 1.2e-5 after 20 iterations; every other component of the error stayed at the fp32 torch evaluation's 2.5e-6).  The sums stay fp32.
__device__ __forceinline__ float sg_potential(float M, float tot, float xd, int m, int n, int marg) {
  const float M2 = fmaxf(M, xd);
  const float t2 = tot * expf(M - M2) + expf(xd - M2);
  const double lse = (double)M2 + log((double)t2);
  const double log_marg = (marg > 0 ? log((double)marg) : 0.0) - log((double)(m + n));   // log_mu / log_nu (SGN:179-181); marg: the dustbin's mass
  return (float)(log_marg - lse);
}

// u[i] = log_mu[i] - LSE_j(Z[i][j] + v[j]), i = 0 .. m (m = the dustbin row).  One wave per row, four per workgroup.
__global__ __launch_bounds__(256) void sg_sinkhorn_rows_kernel(LgState st, SgOt ot) {
  const int p = blockIdx.y;
  if (st.done[p] != 0) return;
  const int m = st.n_cur[2 * p], n = st.n_cur[2 * p + 1], N = st.nmax;
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i > m) return;
  const bool bin = i == m;
  const float* S = st.sim + (size_t)p * N * N + (size_t)(bin ? 0 : i) * N;
  const float* v = ot.v + (size_t)p * (N + 1);
  float mx = -INFINITY, sm = 0.0f;
  for (int j0 = lane * 4; j0 < n; j0 += 256) {   // j0 + 3 <= N - 1: N is a multiple of 4
    float z[4] = {ot.alpha, ot.alpha, ot.alpha, ot.alpha};
    if (!bin) { const float4 q = *(const float4*)(S + j0); z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w; }
    float x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = (j0 + k < n) ? z[k] + v[j0 + k] : -INFINITY;
    lse_fold4(mx, sm, x);
  }
  const float M = wave_max(mx);                      // finite: lane 0 holds column 0
  const float tot = wave_sum(sm * expf(mx - M));     // idle lanes: 0 * exp(-inf) = 0
  if (lane == 0) ot.u[(size_t)p * (N + 1) + i] = sg_potential(M, tot, ot.alpha + v[n], m, n, bin ? n : 0);
}

constexpr int CT = 16, CG = 32;   // columns per workgroup, row groups (512 threads)
// v[j] = log_nu[j] - LSE_i(Z[i][j] + u[i]), j = 0 .. n (n = the dustbin column)
__global__ __launch_bounds__(CT * CG) void sg_sinkhorn_cols_kernel(LgState st, SgOt ot) {
  __shared__ float pm[CG][CT], ps[CG][CT];
  const int p = blockIdx.y;
  if (st.done[p] != 0) return;
  const int m = st.n_cur[2 * p], n = st.n_cur[2 * p + 1], N = st.nmax;
  if ((int)blockIdx.x * CT > n) return;
  const int c = threadIdx.x & (CT - 1), g = threadIdx.x / CT, j = blockIdx.x * CT + c;
  const bool live = j <= n, bin = j == n;
  const float* S = st.sim + (size_t)p * N * N + (bin ? 0 : j);
  const float* u = ot.u + (size_t)p * (N + 1);
  float mx = -INFINITY, sm = 0.0f;
  if (live)
    for (int i0 = g; i0 < m; i0 += 4 * CG) {
      float x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + CG * k;
        x[k] = -INFINITY;
        if (i < m) x[k] = (bin ? ot.alpha : S[(size_t)i * N]) + u[i];
      }
      lse_fold4(mx, sm, x);
    }
  pm[g][c] = mx; ps[g][c] = sm;
  __syncthreads();
  if (g == 0 && live) {
    float M = pm[0][c];   // finite: m >= 1
#pragma unroll
    for (int k = 1; k < CG; ++k) M = fmaxf(M, pm[k][c]);
    float tot = 0.0f;
#pragma unroll
    for (int k = 0; k < CG; ++k) tot += ps[k][c] * expf(pm[k][c] - M);
    ot.v[(size_t)p * (N + 1) + j] = sg_potential(M, tot, ot.alpha + u[m], m, n, bin ? m : 0);
  }
}

// Z - norm at (i, j) exactly as the reference's fp32 evaluation forms it: ((S + u) + v) - norm (SGN:160,185)
__device__ __forceinline__ float sg_z(float s, float ui, float vj, float norm) { return ((s + ui) + vj) - norm; }
__device__ __forceinline__ bool sg_better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// row maximum and argmax over the real block; one wave per row
__global__ __launch_bounds__(256) void sg_row_argmax_kernel(LgState st, SgOt ot) {
  const int p = blockIdx.y;
  if (st.done[p] != 0) return;
  const int m = st.n_cur[2 * p], n = st.n_cur[2 * p + 1], N = st.nmax;
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m) return;
  const float* S = st.sim + (size_t)p * N * N + (size_t)i * N;
  const float* v = ot.v + (size_t)p * (N + 1);
  const float ui = ot.u[(size_t)p * (N + 1) + i], norm = -logf((float)(m + n));
  float best = -INFINITY; int arg = 0x7fffffff;
  for (int j0 = lane * 4; j0 < n; j0 += 256) {
    const float4 q = *(const float4*)(S + j0);
    const float z[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j0 + k < n) {
        const float y = sg_z(z[k], ui, v[j0 + k], norm);
        if (sg_better(y, j0 + k, best, arg)) { best = y; arg = j0 + k; }
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o); const int oa = __shfl_xor(arg, o);
    if (sg_better(ob, oa, best, arg)) { best = ob; arg = oa; }
  }
  if (lane == 0) { ot.arg0[(size_t)p * N + i] = arg; ot.val0[(size_t)p * N + i] = best; }
}

// column argmax over the real block; the layout of sg_sinkhorn_cols_kernel
__global__ __launch_bounds__(CT * CG) void sg_col_argmax_kernel(LgState st, SgOt ot) {
  __shared__ float pb[CG][CT];
  __shared__ int pa[CG][CT];
  const int p = blockIdx.y;
  if (st.done[p] != 0) return;
  const int m = st.n_cur[2 * p], n = st.n_cur[2 * p + 1], N = st.nmax;
  if ((int)blockIdx.x * CT >= n) return;
  const int c = threadIdx.x & (CT - 1), g = threadIdx.x / CT, j = blockIdx.x * CT + c;
  const bool live = j < n;
  const float* S = st.sim + (size_t)p * N * N + (live ? j : 0);
  const float* u = ot.u + (size_t)p * (N + 1);
  const float vj = live ? ot.v[(size_t)p * (N + 1) + j] : 0.0f, norm = -logf((float)(m + n));
  float best = -INFINITY; int arg = 0x7fffffff;
  if (live)
    for (int i = g; i < m; i += CG) {
      const float y = sg_z(S[(size_t)i * N], u[i], vj, norm);
      if (sg_better(y, i, best, arg)) { best = y; arg = i; }
    }
  pb[g][c] = best; pa[g][c] = arg;
  __syncthreads();
  if (g == 0 && live) {
    for (int k = 1; k < CG; ++k)
      if (sg_better(pb[k][c], pa[k][c], best, arg)) { best = pb[k][c]; arg = pa[k][c]; }
    ot.arg1[(size_t)p * N + j] = arg;
  }
}

// mutual check, threshold, matches0 / matches1 and the compact list (ascending in index 0); one workgroup per pair
__global__ __launch_bounds__(256) void sg_finalize_kernel(LgState st, SgOt ot, float thr, int out_cap, long long* __restrict__ matches,
                                                          float* __restrict__ mscores, int* __restrict__ n_matches, int* __restrict__ mfull,
                                                          float* __restrict__ msfull) {
  __shared__ int wtot[4];
  __shared__ int base_s;
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6, N = st.nmax;
  const bool empty = st.done[p] != 0;
  const int m = empty ? 0 : st.n_cur[2 * p], n = empty ? 0 : st.n_cur[2 * p + 1];
  const int* a0 = ot.arg0 + (size_t)p * N; const int* a1 = ot.arg1 + (size_t)p * N;
  const float* v0 = ot.val0 + (size_t)p * N;
  int* m0 = mfull + (size_t)p * 2 * out_cap; int* m1 = m0 + out_cap;
  float* s0 = msfull + (size_t)p * 2 * out_cap; float* s1 = s0 + out_cap;
  if (t == 0) base_s = 0;
  __syncthreads();
  for (int i0 = 0; i0 < out_cap; i0 += 256) {
    const int i = i0 + t;
    int j = -1; float sc = 0.0f; bool valid = false;
    if (i < m) {
      j = a0[i];
      if ((unsigned)j >= (unsigned)n) j = -1;   // (a row of NaNs has no maximum)
      else if (a1[j] == i) { sc = expf(v0[i]); valid = sc > thr; }
    }
    if (i < out_cap) { m0[i] = valid ? j : -1; s0[i] = sc; }
    const unsigned long long bal = __ballot(valid);
    if (lane == 0) wtot[wv] = __popcll(bal);
    __syncthreads();
    int off = base_s;
    for (int k = 0; k < wv; ++k) off += wtot[k];
    if (valid) {
      const int dst = off + __popcll(bal & ((1ull << lane) - 1ull));
      matches[((size_t)p * out_cap + dst) * 2] = i; matches[((size_t)p * out_cap + dst) * 2 + 1] = j;
      mscores[(size_t)p * out_cap + dst] = sc;
    }
    __syncthreads();
    if (t == 0) base_s += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (t == 0) n_matches[p] = base_s;
  for (int j = t; j < out_cap; j += 256) {   // matching_scores1 is gathered from side 0 (SGN:294-296)
    int i = -1; float sc = 0.0f; bool valid = false;
    if (j < n) {
      i = a1[j];
      if ((unsigned)i >= (unsigned)m) i = -1;
      else if (a0[i] == j) { sc = expf(v0[i]); valid = sc > thr; }
    }
    m1[j] = valid ? i : -1; s1[j] = sc;
  }
}
}  // namespace

int launch_sg_encoder(const LgState& st, const SgEncW& w, const float* kpts_tab, const float* desc_tab, const float* score_tab, const int* n_tab,
                      const float* size_tab, const int* pair_idx, int cap, unsigned* sat, hipStream_t s) {
  hipLaunchKernelGGL(sg_encoder_kernel, dim3(cdiv(st.nsel, ET), st.n_items), dim3(256), 0, s, st, w, kpts_tab, desc_tab, score_tab, n_tab, size_tab,
                     pair_idx, cap, sat);
  DIM_LAUNCH_CHECK();
  return 0;
}
int launch_sg_sinkhorn_rows(const LgState& st, const SgOt& ot, hipStream_t s) {
  hipLaunchKernelGGL(sg_sinkhorn_rows_kernel, dim3(cdiv(st.nsel + 1, 4), st.n_pairs), dim3(256), 0, s, st, ot);
  DIM_LAUNCH_CHECK();
  return 0;
}
int launch_sg_sinkhorn_cols(const LgState& st, const SgOt& ot, hipStream_t s) {
  hipLaunchKernelGGL(sg_sinkhorn_cols_kernel, dim3(cdiv(st.nsel + 1, CT), st.n_pairs), dim3(CT * CG), 0, s, st, ot);
  DIM_LAUNCH_CHECK();
  return 0;
}
int launch_sg_select(const LgState& st, const SgOt& ot, float thr, int out_cap, long long* matches, float* mscores, int* n_matches, int* mfull,
                     float* msfull, hipStream_t s) {
  hipLaunchKernelGGL(sg_row_argmax_kernel, dim3(cdiv(st.nsel, 4), st.n_pairs), dim3(256), 0, s, st, ot);
  DIM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sg_col_argmax_kernel, dim3(cdiv(st.nsel, CT), st.n_pairs), dim3(CT * CG), 0, s, st, ot);
  DIM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sg_finalize_kernel, dim3(st.n_pairs), dim3(256), 0, s, st, ot, thr, out_cap, matches, mscores, n_matches, mfull, msfull);
  DIM_LAUNCH_CHECK();
  return 0;
}
