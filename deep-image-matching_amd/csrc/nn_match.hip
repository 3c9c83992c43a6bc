// Nearest-neighbour descriptor matching (kornia.feature.DescriptorMatcher's nn / mnn / snn / smnn, the reference's
// matchers/kornia_matcher.py) for a batch of image pairs addressed through a feature table, without ever storing the M x N
// distance matrix:
//   nn_owner_kernel     which (pair, side) item computes the norms of its image slot (the first one that names the slot)
//   nn_norms_kernel     |x|^2 of every live descriptor row, fp32, fixed summation order, once per image slot; range guard
//   nn_tile_kernel      one workgroup = one 128 x 128 tile of s = A B^T in the split arithmetic of gemm_x6_nt_kernel, turned into
//                       d^2 = max(|a|^2 + |b|^2 - 2 s, 0) in registers and reduced to (min d^2, argmin, second-smallest d^2) per
//                       row and per column of the tile: only these partial triples are written
//   nn_merge_kernel     partial triples of the tiles of a row / of a column -> the final triple (ascending tile order)
//   nn_finalize_kernel  the mode's tests + the compact idx0-ascending match list (prefix scan), one workgroup per pair
// Ties on equal d^2 go to the lowest index everywhere; there is no atomic on the selection, so results repeat bit for bit.
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "../../include/dim_hip.h"
#include "dim_kernels.h"

namespace {
constexpr int KC = 32, RS = 20, BT = 128;   // K chunk, row stride in dwords of a staged split chunk (gemm_x6.hip), tile edge
constexpr int RSF = KC + 4;                 // row stride in floats of a staged fp32 chunk

struct NnArgs {
  const float* desc; const int* n_tab; const int* pair_idx;
  int cap, D, NK, T, TL;              // table rows per image, descriptor dimension, handle row stride, tiles per NK rows (strides), tiles per side of THIS launch
  const int* owner; const float* norms;   // [2 max_pairs], [2 max_pairs][NK]
  float* rp; float* cp;               // partial triples: rows [P][T][3][NK] (over column tiles), columns [P][T][3][NK] (over row tiles)
  float* fin;                         // final triples [P][2][3][NK]: plane 0 = argmin (int32 bits), 1 = min d^2, 2 = second d^2
};
__device__ __forceinline__ int nn_slot(const NnArgs& a, int item) { return a.pair_idx ? a.pair_idx[item] : item; }
__device__ __forceinline__ int nn_count(const NnArgs& a, int item) { return max(0, min(a.n_tab[nn_slot(a, item)], min(a.cap, a.NK))); }

// (min d^2, its index, second-smallest d^2) of a set of candidates; the empty set is (inf, INT_MAX, inf)
struct Tri { float b; int i; float s; };
__device__ __forceinline__ Tri tri_empty() { return Tri{INFINITY, INT_MAX, INFINITY}; }
// a candidate whose index is above every index already in t
__device__ __forceinline__ void tri_insert(Tri& t, float v, int idx) {
  const bool lt = v < t.b;
  t.s = lt ? t.b : fminf(t.s, v);
  t.i = lt ? idx : t.i;
  t.b = lt ? v : t.b;
}
// union of two disjoint candidate sets, in any order: equal minima keep the lower index
__device__ __forceinline__ Tri tri_merge(const Tri& x, const Tri& y) {
  const bool ty = y.b < x.b || (y.b == x.b && y.i < x.i);
  Tri r;
  r.b = ty ? y.b : x.b;
  r.i = ty ? y.i : x.i;
  r.s = fminf(ty ? x.b : y.b, fminf(x.s, y.s));
  return r;
}
// the value lane ^ X holds: DPP quad permutes for X = 1, 2 (no LDS traffic), ds_bpermute beyond
template <int X> __device__ __forceinline__ int lane_xchg_i(int v) {
  if constexpr (X == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
  else if constexpr (X == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
  else return __shfl_xor(v, X);
}
template <int X> __device__ __forceinline__ Tri tri_xchg(const Tri& t) {
  return Tri{__int_as_float(lane_xchg_i<X>(__float_as_int(t.b))), lane_xchg_i<X>(t.i), __int_as_float(lane_xchg_i<X>(__float_as_int(t.s)))};
}
// One step of the transposing reduction over the 32 lanes of a tile column group: the lanes with bit X of their number clear keep the
// lower half of the HS * 2 live triples, the others the upper half, and each hands the half it drops to its partner lane ^ X — half
// the triples, each over twice the lanes.  31 exchanges reduce 32 rows over 32 lanes (a butterfly per row would take 160).
template <int X, int HS> __device__ __forceinline__ void tri_fold(Tri (&T)[32], int lx) {
  const bool up = (lx & X) != 0;
#pragma unroll
  for (int k = 0; k < HS; ++k) {
    const Tri lo = T[k], hi = T[k + HS];
    const Tri mine = up ? hi : lo, give = up ? lo : hi;
    T[k] = tri_merge(mine, tri_xchg<X>(give));
  }
}

__global__ void nn_owner_kernel(const int* pair_idx, int n_items, int* owner) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_items) return;
  const int s = pair_idx ? pair_idx[k] : k;
  int o = k;
  for (int j = 0; j < k; ++j)
    if ((pair_idx ? pair_idx[j] : j) == s) { o = j; break; }
  owner[k] = o;
}

// 16 lanes per row: lane q sums the squares of its float4 groups q, q + 16, ... in order, the 16 partial sums are added by four DPP steps
__global__ __launch_bounds__(256) void nn_norms_kernel(NnArgs a, float* norms, unsigned* sat) {
  const int item = blockIdx.y;
  if (a.owner[item] != item) return;
  const int n = nn_count(a, item);
  if ((int)blockIdx.x * 16 >= n) return;
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), q = threadIdx.x & 15;
  const float* p = a.desc + ((size_t)nn_slot(a, item) * a.cap + min(row, n - 1)) * a.D;
  float acc = 0.0f;
  bool bad = false;
  for (int c = q * 4; c < a.D; c += 64) {
    const float4 v = *(const float4*)(p + c);
    acc += v.x * v.x; acc += v.y * v.y; acc += v.z * v.z; acc += v.w * v.w;
    // NaN-sticky: an external input may hold anything
    bad |= !(fabsf(v.x) <= DIM_F16_ACT_LIMIT) | !(fabsf(v.y) <= DIM_F16_ACT_LIMIT) | !(fabsf(v.z) <= DIM_F16_ACT_LIMIT) | !(fabsf(v.w) <= DIM_F16_ACT_LIMIT);
  }
  acc += dpp_f(acc, 0xB1);
  acc += dpp_f(acc, 0x4E);
  acc += dpp_f(acc, 0x141);
  acc += dpp_f(acc, 0x140);
  if (q == 0 && row < n) norms[(size_t)item * a.NK + row] = acc;
  if (sat != nullptr && bad) atomicAdd(sat, 1u);
}

struct NnTile { int p, M, N, m0, n0, tm, tn; };
// XCD-aware tile order (conv_x6.hip): the hardware sends workgroup L to XCD L % 8; every XCD gets a contiguous band of the
// row-major tile list, so the tiles that share descriptor rows of image 0 find them in that XCD's L2.  Speed only.
__device__ __forceinline__ bool nn_pick_tile(const NnArgs& a, NnTile& t) {
  const int nt = gridDim.x, xcd = blockIdx.x & 7, j = blockIdx.x >> 3, q = nt >> 3, r = nt & 7;
  const int tile = xcd * q + min(xcd, r) + j;
  t.p = blockIdx.y;
  t.M = nn_count(a, 2 * t.p); t.N = nn_count(a, 2 * t.p + 1);
  t.tm = tile / a.TL; t.tn = tile % a.TL;
  t.m0 = t.tm * BT; t.n0 = t.tn * BT;
  return t.m0 < t.M && t.n0 < t.N;
}
__device__ __forceinline__ void nn_stage_norms(const NnArgs& a, const NnTile& t, float* na, float* nb) {
  const int x = threadIdx.x;
  if (x < BT) na[x] = t.m0 + x < t.M ? a.norms[(size_t)a.owner[2 * t.p] * a.NK + t.m0 + x] : INFINITY;
  else nb[x - BT] = t.n0 + x - BT < t.N ? a.norms[(size_t)a.owner[2 * t.p + 1] * a.NK + t.n0 + x - BT] : INFINITY;
}

// acc[m][n]: the wave's 64 x 64 block of s (times 1 / inv) in the 32 x 32 accumulator layout (lane: column lx, rows mfma_row(r, half)).
// A column's candidates lie in the lane's own registers (then lane ^ 32, then the other row wave through LDS); a row's candidates lie
// across the 32 lanes (tri_fold), then the other column wave through LDS.  Rows / columns past the ragged end carry an infinite norm.
__device__ __forceinline__ void nn_tile_epilogue(const NnArgs& a, const NnTile& t, f32x16 (&acc)[2][2], float inv, const float* na, const float* nb,
                                                 float (*xr)[3][BT], float (*xc)[3][BT]) {
  const int x = threadIdx.x, lane = x & 63, wv = x >> 6, wm = wv >> 1, wn = wv & 1, lx = lane & 31, half = lane >> 5;
  float nbv[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) nbv[n] = nb[wn * 64 + n * 32 + lx];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float nav = na[wm * 64 + m * 32 + mfma_row(r, half)];
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n][r] = fmaxf((nav + nbv[n]) - 2.0f * (acc[m][n][r] * inv), 0.0f);
    }
  // columns
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    Tri c = tri_empty();
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) tri_insert(c, acc[m][n][r], t.m0 + wm * 64 + m * 32 + mfma_row(r, half));
    c = tri_merge(c, tri_xchg<32>(c));
    if (half == 0) {
      const int cl = wn * 64 + n * 32 + lx;
      xc[wm][0][cl] = __int_as_float(c.i); xc[wm][1][cl] = c.b; xc[wm][2][cl] = c.s;
    }
  }
  // rows
  Tri T[32];
  const int c0 = t.n0 + wn * 64 + lx;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      Tri v{acc[m][0][r], c0, INFINITY};
      tri_insert(v, acc[m][1][r], c0 + 32);
      T[m * 16 + r] = v;
    }
  tri_fold<1, 16>(T, lx);
  tri_fold<2, 8>(T, lx);
  tri_fold<4, 4>(T, lx);
  tri_fold<8, 2>(T, lx);
  tri_fold<16, 1>(T, lx);
  {
    const int q = ((lx & 1) << 4) | ((lx & 2) << 2) | (lx & 4) | ((lx & 8) >> 2) | ((lx & 16) >> 4);
    const int rl = wm * 64 + (q >> 4) * 32 + mfma_row(q & 15, half);
    xr[wn][0][rl] = __int_as_float(T[0].i); xr[wn][1][rl] = T[0].b; xr[wn][2][rl] = T[0].s;
  }
  __syncthreads();
  const bool is_row = x < BT;
  const int e = is_row ? x : x - BT;
  float (*src)[3][BT] = is_row ? xr : xc;
  const Tri lo{src[0][1][e], __float_as_int(src[0][0][e]), src[0][2][e]}, hi{src[1][1][e], __float_as_int(src[1][0][e]), src[1][2][e]};
  const Tri f = tri_merge(lo, hi);
  const int g = (is_row ? t.m0 : t.n0) + e;
  if (g < (is_row ? t.M : t.N)) {
    float* dst = (is_row ? a.rp : a.cp) + ((size_t)t.p * a.T + (is_row ? t.tn : t.tm)) * 3 * a.NK;
    dst[g] = __int_as_float(f.i); dst[a.NK + g] = f.b; dst[2 * (size_t)a.NK + g] = f.s;
  }
}

// MODE 1 = bf16x6, 2 = fp16x3 (SplitMma, dim_common.h); ONE (fp16x3 only): the table holds fp16-exact values, whose low pieces are zero —
// only the high plane is staged and one MFMA term runs instead of three (the two dropped terms add exact zeros: same bits).
template <int MODE, bool ONE>
__global__ __launch_bounds__(256, 2) void nn_tile_kernel(NnArgs a) {
  using S = SplitMma<MODE>;
  constexpr int NPL = ONE ? 1 : S::NPL, NTERM = ONE ? 1 : S::NT;
  __shared__ unsigned Ap[NPL * BT * RS], Bp[NPL * BT * RS];
  __shared__ float na[BT], nb[BT], xr[2][3][BT], xc[2][3][BT];
  NnTile tl;
  if (!nn_pick_tile(a, tl)) return;
  nn_stage_norms(a, tl, na, nb);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv >> 1, wn = wv & 1, lx = lane & 31, half = lane >> 5;
  const float* A = a.desc + (size_t)nn_slot(a, 2 * tl.p) * a.cap * a.D;
  const float* B = a.desc + (size_t)nn_slot(a, 2 * tl.p + 1) * a.cap * a.D;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  float4 ra[4], rb[4];
  auto load_chunk = [&](int k0) {   // rows past the ragged end re-read the last valid one (their norm is infinite)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = t + 256 * i, row = idx >> 3, q = idx & 7;
      ra[i] = *(const float4*)(A + (size_t)min(tl.m0 + row, tl.M - 1) * a.D + k0 + q * 4);
      rb[i] = *(const float4*)(B + (size_t)min(tl.n0 + row, tl.N - 1) * a.D + k0 + q * 4);
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = t + 256 * i, row = idx >> 3, q = idx & 7;
      unsigned p0[S::NPL], p1[S::NPL], q0[S::NPL], q1[S::NPL];
      S::split(ra[i].x, ra[i].y, S::act_scale(), p0); S::split(ra[i].z, ra[i].w, S::act_scale(), p1);
      S::split(rb[i].x, rb[i].y, S::act_scale(), q0); S::split(rb[i].z, rb[i].w, S::act_scale(), q1);
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        Ap[(pl * BT + row) * RS + q * 2] = p0[pl]; Ap[(pl * BT + row) * RS + q * 2 + 1] = p1[pl];
        Bp[(pl * BT + row) * RS + q * 2] = q0[pl]; Bp[(pl * BT + row) * RS + q * 2 + 1] = q1[pl];
      }
    }
  };
  load_chunk(0);
  for (int k0 = 0; k0 < a.D; k0 += KC) {
    store_chunk();
    __syncthreads();
    load_chunk(min(k0 + KC, a.D - KC));
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 fa[2][NPL], fb[2][NPL];
#pragma unroll
      for (int p = 0; p < NPL; ++p)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          fa[m][p] = *(const u32x4*)&Ap[(p * BT + wm * 64 + m * 32 + lx) * RS + ks * 8 + half * 4];
          fb[m][p] = *(const u32x4*)&Bp[(p * BT + wn * 64 + m * 32 + lx) * RS + ks * 8 + half * 4];
        }
#pragma unroll
      for (int tm = 0; tm < NTERM; ++tm)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n) acc[m][n] = S::mma(fa[m][ONE ? 0 : S::ta(tm)], fb[n][ONE ? 0 : S::tb(tm)], acc[m][n]);
    }
    __syncthreads();
  }
  nn_tile_epilogue(a, tl, acc, 1.0f / (S::act_scale() * S::act_scale()), na, nb, xr, xc);
}

// dim_tune_set key 1 = 0: the same tile on the fp32 MFMA (v_mfma_f32_32x32x2_f32)
__global__ __launch_bounds__(256, 2) void nn_tile_f32_kernel(NnArgs a) {
  __shared__ float As[BT * RSF], Bs[BT * RSF];
  __shared__ float na[BT], nb[BT], xr[2][3][BT], xc[2][3][BT];
  NnTile tl;
  if (!nn_pick_tile(a, tl)) return;
  nn_stage_norms(a, tl, na, nb);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv >> 1, wn = wv & 1, lx = lane & 31, half = lane >> 5;
  const float* A = a.desc + (size_t)nn_slot(a, 2 * tl.p) * a.cap * a.D;
  const float* B = a.desc + (size_t)nn_slot(a, 2 * tl.p + 1) * a.cap * a.D;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  for (int k0 = 0; k0 < a.D; k0 += KC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = t + 256 * i, row = idx >> 3, q = idx & 7;
      *(float4*)&As[row * RSF + q * 4] = *(const float4*)(A + (size_t)min(tl.m0 + row, tl.M - 1) * a.D + k0 + q * 4);
      *(float4*)&Bs[row * RSF + q * 4] = *(const float4*)(B + (size_t)min(tl.n0 + row, tl.N - 1) * a.D + k0 + q * 4);
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < KC; kk += 2) {
      float fa[2], fb[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        fa[m] = As[(wm * 64 + m * 32 + lx) * RSF + kk + half];
        fb[m] = Bs[(wn * 64 + m * 32 + lx) * RSF + kk + half];
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = mfma32(fa[m], fb[n], acc[m][n]);
    }
    __syncthreads();
  }
  nn_tile_epilogue(a, tl, acc, 1.0f, na, nb, xr, xc);
}

// grid (row blocks, side, pair): side 0 merges the partial triples of a row over the column tiles, side 1 those of a column over the row tiles
__global__ __launch_bounds__(256) void nn_merge_kernel(NnArgs a, float* row_tap, float* col_tap) {
  const int p = blockIdx.z, side = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int M = nn_count(a, 2 * p), N = nn_count(a, 2 * p + 1);
  const int cnt = side ? N : M, other = side ? M : N;
  if (i >= cnt) return;
  const int ntile = (other + BT - 1) / BT;
  const float* part = (side ? a.cp : a.rp) + (size_t)p * a.T * 3 * a.NK;
  Tri f = tri_empty();
  for (int tl = 0; tl < ntile; ++tl) {
    const float* q = part + (size_t)tl * 3 * a.NK;
    f = tri_merge(f, Tri{q[a.NK + i], __float_as_int(q[i]), q[2 * (size_t)a.NK + i]});
  }
  float* dst = a.fin + ((size_t)p * 2 + side) * 3 * a.NK;
  dst[i] = __int_as_float(f.i); dst[a.NK + i] = f.b; dst[2 * (size_t)a.NK + i] = f.s;
  float* tap = side ? col_tap : row_tap;
  if (tap != nullptr) {
    tap += (size_t)p * 3 * a.NK;
    tap[i] = __int_as_float(f.i); tap[a.NK + i] = f.b; tap[2 * (size_t)a.NK + i] = f.s;
  }
}

// d_best / d_second of kornia's ratio test (match_snn: vals[:, 0] / vals[:, 1] on the distances); 0 / 0 is NaN and fails every comparison
__device__ __forceinline__ float nn_ratio(float best, float second) { return sqrtf(best) / sqrtf(second); }

// mode 0 nn, 1 mnn, 2 snn, 3 smnn.  One workgroup per pair walks the rows in order; a ballot + popcount prefix keeps the list idx0-ascending.
__global__ __launch_bounds__(256) void nn_finalize_kernel(NnArgs a, int mode, float th, long long* matches, float* dists, int* n_matches) {
  __shared__ int wave_cnt[4];
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int M = nn_count(a, 2 * p), N = nn_count(a, 2 * p + 1);
  const float* fr = a.fin + (size_t)p * 2 * 3 * a.NK;
  const float* fc = fr + 3 * (size_t)a.NK;
  const bool enough = mode == 2 ? N >= 2 : (mode == 3 ? (M >= 2 && N >= 2) : N >= 1);
  int base = 0;
  for (int i0 = 0; i0 < M && enough; i0 += 256) {
    const int i = i0 + t;
    bool ok = false;
    int j = 0;
    float dist = 0.0f;
    if (i < M) {
      j = __float_as_int(fr[i]);
      const float rb = fr[a.NK + i], rs = fr[2 * (size_t)a.NK + i];
      ok = j >= 0 && j < N;
      const int jc = ok ? j : 0;
      if (mode == 0 || mode == 1) {
        dist = sqrtf(fmaxf(rb, 1e-30f));
        if (mode == 1) ok = ok && __float_as_int(fc[jc]) == i;
      } else {
        const float r0 = nn_ratio(rb, rs);
        ok = ok && r0 <= th;
        dist = r0;
        if (mode == 3) {
          const float r1 = nn_ratio(fc[a.NK + jc], fc[2 * (size_t)a.NK + jc]);
          ok = ok && __float_as_int(fc[jc]) == i && r1 <= th;
          dist = fmaxf(r0, r1);
        }
      }
    }
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { before += w < wv ? wave_cnt[w] : 0; total += wave_cnt[w]; }
    if (ok) {
      const size_t pos = (size_t)p * a.NK + base + before + __popcll(bal & ((1ull << lane) - 1ull));
      matches[2 * pos] = i; matches[2 * pos + 1] = j;
      dists[pos] = dist;
    }
    base += total;
    __syncthreads();
  }
  if (t == 0) n_matches[p] = base;
}
}  // namespace

struct dim_nn {
  DimHandleBase base;
  dim_nn_config cfg;
  int max_pairs = 0, nk = 0, dim = 0, T = 0;
  int* owner = nullptr;
  float *norms = nullptr, *rp = nullptr, *cp = nullptr, *fin = nullptr;
};

extern "C" {

void dim_nn_destroy(dim_nn* h) {
  if (!h) return;
  dim_handle_release(&h->base);
  delete h;
}

int dim_nn_create(const dim_nn_config* cfg, int max_pairs, int max_kpts, int dim, dim_nn** out) {
  DIM_REQUIRE(cfg && out, "dim_nn_create: null argument");
  DIM_REQUIRE(cfg->mode >= DIM_NN_MODE_NN && cfg->mode <= DIM_NN_MODE_SMNN, "dim_nn_create: mode %d (0 nn, 1 mnn, 2 snn, 3 smnn)", cfg->mode);
  DIM_REQUIRE(max_pairs > 0 && max_kpts > 0, "dim_nn_create: bad sizes");
  DIM_REQUIRE(dim >= 64 && dim % 64 == 0, "dim_nn_create: descriptor dimension %d must be a multiple of 64", dim);
  std::unique_ptr<dim_nn, void (*)(dim_nn*)> guard(new dim_nn(), dim_nn_destroy);
  dim_nn* const h = guard.get();
  DimHandleBase* const hb = &h->base;
  h->cfg = *cfg;
  h->max_pairs = max_pairs; h->dim = dim;
  h->nk = (max_kpts + 3) & ~3;
  h->T = cdiv(h->nk, BT);
  const size_t P = max_pairs, NK = h->nk, T = h->T;
  DIM_TRY(dim_dev_alloc(hb, &h->owner, 2 * P)); DIM_TRY(dim_dev_alloc(hb, &h->norms, 2 * P * NK)); DIM_TRY(dim_dev_alloc(hb, &h->rp, P * T * 3 * NK));
  DIM_TRY(dim_dev_alloc(hb, &h->cp, P * T * 3 * NK)); DIM_TRY(dim_dev_alloc(hb, &h->fin, P * 2 * 3 * NK));
  *out = guard.release();
  return 0;
}

int dim_nn_max_kpts(dim_nn* h) { return h ? h->nk : 0; }
size_t dim_nn_workspace_bytes(dim_nn* h) { return h ? h->base.bytes : 0; }

int dim_nn_match(dim_nn* h, const float* desc_tab_dev, const int32_t* n_tab_dev, int cap, int desc_is_f16_exact, const int32_t* pair_idx_dev,
                 int n_pairs, int64_t* matches_dev, float* dists_dev, int32_t* n_matches_dev, float* row_stats_dev, float* col_stats_dev,
                 void* stream) {
  DIM_REQUIRE(h && desc_tab_dev && n_tab_dev, "dim_nn_match: null input");
  DimTuneScope tune_scope(&h->base);
  DIM_REQUIRE(matches_dev && dists_dev && n_matches_dev, "dim_nn_match: null output");
  DIM_REQUIRE(n_pairs >= 1 && n_pairs <= h->max_pairs, "dim_nn_match: n_pairs %d outside [1,%d]", n_pairs, h->max_pairs);
  DIM_REQUIRE(cap > 0, "dim_nn_match: cap");
  hipStream_t s = (hipStream_t)stream;
  const int pmode = dim_precision_mode();
  NnArgs a;
  a.desc = desc_tab_dev; a.n_tab = n_tab_dev; a.pair_idx = pair_idx_dev;
  a.cap = cap; a.D = h->dim; a.NK = h->nk; a.T = h->T;
  a.owner = h->owner; a.norms = h->norms; a.rp = h->rp; a.cp = h->cp; a.fin = h->fin;
  // launch shapes follow the table's rows per image, not the handle's capacity (kernels exit on the device-side counts)
  const int nsel = std::min(h->nk, cap), items = 2 * n_pairs, tiles = cdiv(nsel, BT);
  a.TL = tiles;
  hipLaunchKernelGGL(nn_owner_kernel, dim3(cdiv(items, 64)), dim3(64), 0, s, pair_idx_dev, items, h->owner);
  DIM_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_norms_kernel, dim3(cdiv(nsel, 16), items), dim3(256), 0, s, a, h->norms, pmode == 2 ? dim_sat_counter(DIM_SAT_OP) : nullptr);
  DIM_LAUNCH_CHECK();
  const dim3 grid(tiles * tiles, n_pairs);
  if (pmode == 2 && desc_is_f16_exact) hipLaunchKernelGGL(HIP_KERNEL_NAME(nn_tile_kernel<2, true>), grid, dim3(256), 0, s, a);
  else if (pmode == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(nn_tile_kernel<2, false>), grid, dim3(256), 0, s, a);
  else if (pmode == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(nn_tile_kernel<1, false>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(nn_tile_f32_kernel, grid, dim3(256), 0, s, a);
  DIM_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_merge_kernel, dim3(cdiv(nsel, 256), 2, n_pairs), dim3(256), 0, s, a, row_stats_dev, col_stats_dev);
  DIM_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_finalize_kernel, dim3(n_pairs), dim3(256), 0, s, a, h->cfg.mode, (float)h->cfg.th, (long long*)matches_dev, dists_dev, n_matches_dev);
  DIM_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
