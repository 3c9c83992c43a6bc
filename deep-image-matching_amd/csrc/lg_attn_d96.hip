// LighterGlue attention: ONE head of dimension 96, on the 16-bit matrix cores at fp32 accuracy (fp16x3 / bf16x6, dim_common.h SplitMma).
// The dataflow is lg_attn_x6.hip's — transposed score tile S^T[key][query] = K·Q^T so that every lane owns one query column, probabilities
// fed back as the B operand of O^T[d][query] += V^T·P^T without leaving registers, log2-domain online softmax with deferred rescale,
// K | V tile images pre-split once per layer and staged by LDS-DMA — at another shape:
//   K·Q^T takes SIX 32x32x16 steps per plane (96 = 6 x 16), O^T is THREE 32-row accumulator blocks (96 = 3 x 32),
//   rotary runs over 48 frequency pairs (enc rows cos[48] | sin[48]), the key-split partials carry 96 + m + l values per query.
//
// Operand images (one 16-B ds_read_b128 = one MFMA operand, consecutive lanes -> consecutive slots):
//   Kp[plane][d-block 12][key 32][8 pieces]       A operand of K·Q^T (k = d): d-block b holds dims 8b .. 8b + 7; step s reads blocks 2s + half
//   Vp[plane][step 2][k-half 2][d 96][8 keys]     A operand of V^T·P^T (k = key), keys in the order in which the MFMA C layout of S^T holds them:
//       register 8u + e of lane-half h holds key (e & 3) + 8 (2u + (e >> 2)) + 4h, so registers 8u .. 8u + 7 of P ARE the B operand of step u
//   Q is split once into registers (6 steps x planes), rotary and the softmax scale applied on load.
// Budget per workgroup (256 threads = 4 waves x 32 queries): two tile images in LDS = 2 x planes x 768 x 16 B = 48 KB (fp16x3) / 72 KB (bf16x6);
// registers: Q 6 x planes x 4, O^T 48, S^T 16, P 16 + fragments (the compiler's figures: DESIGN.md section 5).
#include <math.h>

#include "lg_kernels.h"

namespace {
constexpr int HD = 96, HF = 48, QSTEPS = HD / 16, OBLK = HD / 32, KBLK = HD / 8;
constexpr int PLANE_SLOTS = KBLK * 32;            // 384 16-byte slots per plane for K, and 2 * 2 * 96 = 384 for V
constexpr int TILE_STRIDE96 = 3 * 2 * PLANE_SLOTS;   // slots reserved per (item, 32-key tile) image in HBM (bf16x6 fills all 2304)
constexpr int PART96 = 100;                      // 96 output dims + m + l, padded to a 16-byte multiple

struct AttnArgs96 {
  const float* q; const float* k; const float* v; float* o;
  int ldq, ldk, ldv, ldo;
  long long sq, sk, sv, so;
  const int* n; const int* done;
  int cross;
  float qscale, kscale;  // self: q x 96^-0.5 (LGN:106-108 through scaled_dot_product_attention), k x 1; cross: both x 96^-0.25 (LGN:197-206)
  const float* enc;      // [items][nmax][96] cos[48] | sin[48]; rotary is applied to q and k iff !cross
  u32x4* kv_img;         // [items][tiles][2304] pre-split K | V tile images (kv_prep96_kernel)
  int nmax, tiles;
  int splits;            // key range cut into `splits` parts per (query block, item): small batches only
  int qblocks, groups;   // workgroups per item = qblocks (incl. splits); groups = items (XCD-aware 1-D grid)
  float* part;           // [items][nmax][splits][PART96] partial (unnormalised O, running max, running sum)
  unsigned* sat;         // fp16x3 range guard on the rotated / scaled K and on V
};

// One workgroup per (key tile, item): rotary on K (self-attention only, LGN:41-54,155-156), the split of K and V, written in the LDS-image order.
template <int MODE>
__global__ __launch_bounds__(256) void kv_prep96_kernel(AttnArgs96 a) {
  using S = SplitMma<MODE>;
  constexpr int NPL = S::NPL, KSL = NPL * PLANE_SLOTS;
  const int tile = blockIdx.x, item = blockIdx.y;
  if (a.done[item >> 1] != 0) return;
  const int nk = a.n[item], kt = tile * 32;
  if (kt >= nk) return;
  const float* kb = a.k + (size_t)item * a.sk;
  const float* vb = a.v + (size_t)item * a.sv;
  u32x4* img = a.kv_img + ((size_t)item * a.tiles + tile) * TILE_STRIDE96;
  float vmax = 0.0f;
  for (int w = threadIdx.x; w < PLANE_SLOTS; w += 256) {  // K: (key = w / 12, d-block = w % 12: dims 8 blk .. 8 blk + 7 = frequency pairs 4 blk .. 4 blk + 3)
    const int key = w / KBLK, blk = w - key * KBLK;
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (kt + key < nk) {
      const float* p = kb + (size_t)(kt + key) * a.ldk + 8 * blk;
      const float4 x0 = *(const float4*)p, x1 = *(const float4*)(p + 4);
      x[0] = x0.x; x[1] = x0.y; x[2] = x0.z; x[3] = x0.w; x[4] = x1.x; x[5] = x1.y; x[6] = x1.z; x[7] = x1.w;
      if (!a.cross) {
        const float* e = a.enc + ((size_t)item * a.nmax + kt + key) * HD + 4 * blk;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float c = e[i], sn = e[HF + i], t0 = x[2 * i], t1 = x[2 * i + 1];
          x[2 * i] = t0 * c + (-t1) * sn;
          x[2 * i + 1] = t1 * c + t0 * sn;
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] *= a.kscale;
    }
    unsigned pc[4][NPL];
#pragma unroll
    for (int i = 0; i < 4; ++i) { S::split(x[2 * i], x[2 * i + 1], S::act_scale(), pc[i]); vmax = sat_track(vmax, x[2 * i], x[2 * i + 1]); }
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) img[(pl * KBLK + blk) * 32 + key] = u32x4{pc[0][pl], pc[1][pl], pc[2][pl], pc[3][pl]};
  }
  for (int w = threadIdx.x; w < PLANE_SLOTS; w += 256) {  // V: (d = w % 96, step u, k-half hh), keys in MFMA-C-layout order
    const int uh = w / HD, d = w - uh * HD, u = uh >> 1, hh = uh & 1;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int key = (e & 3) + 8 * (2 * u + (e >> 2)) + 4 * hh;
      x[e] = (kt + key < nk) ? vb[(size_t)(kt + key) * a.ldv + d] : 0.0f;
    }
    unsigned pc[4][NPL];
#pragma unroll
    for (int i = 0; i < 4; ++i) { S::split(x[2 * i], x[2 * i + 1], S::act_scale(), pc[i]); vmax = sat_track(vmax, x[2 * i], x[2 * i + 1]); }
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) img[KSL + ((pl * 2 + u) * 2 + hh) * HD + d] = u32x4{pc[0][pl], pc[1][pl], pc[2][pl], pc[3][pl]};
  }
  if (MODE == 2) sat_report(a.sat, vmax);
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void attn_d96_kernel(AttnArgs96 a) {
  using S = SplitMma<MODE>;
  constexpr int NPL = S::NPL, TILE_SLOTS = NPL * 2 * PLANE_SLOTS, KSL = NPL * PLANE_SLOTS, NCP = TILE_SLOTS / 256;
  static_assert(TILE_SLOTS % 256 == 0, "a tile image is staged in whole rounds of 256 lanes");
  // K, Q, V and P are multiplied by the (power-of-two) activation scale before the split: exact factors
  const float inv_qk = 1.0f / (S::act_scale() * S::act_scale());
  // XCD-aware mapping of the 1-D grid (lg_attn_x6.hip): all query blocks of one item stream the same tile images -> one XCD's L2
  const int L = blockIdx.x, xcd = L & 7, slot = L >> 3;
  const int item = (slot / a.qblocks) * 8 + xcd, bx = slot % a.qblocks;
  if (item >= a.groups) return;
  const int qb = bx / a.splits, sp = bx - qb * a.splits, q0 = qb * 128;
  if (a.done[item >> 1] != 0) return;
  const int kitem = a.cross ? (item ^ 1) : item;
  const int nq = a.n[item], nk = a.n[kitem];
  if (q0 >= nq) return;

  // two tile images: the next key tile arrives by LDS-DMA in the other half while this one is consumed — one barrier per tile
  __shared__ u32x4 img[2 * TILE_SLOTS];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lx = lane & 31, half = lane >> 5;
  const int qrow = q0 + wv * 32 + lx;
  const bool qok = qrow < nq;

  // Q^T operand: lane (query lx, half) holds dims 16s + 8 half + 0..7 for s = 0..5 (the K image's assignment), NPL planes each
  u32x4 qf[QSTEPS][NPL];
  const float sc = a.qscale * 1.44269504088896340736f;  // scores in the log2 domain
  {
    const float* qp = a.q + (size_t)item * a.sq + (size_t)(qok ? qrow : 0) * a.ldq + half * 8;
#pragma unroll
    for (int s = 0; s < QSTEPS; ++s) {
      float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (qok) {
        const float4 x0 = *(const float4*)(qp + 16 * s), x1 = *(const float4*)(qp + 16 * s + 4);
        x[0] = x0.x; x[1] = x0.y; x[2] = x0.z; x[3] = x0.w; x[4] = x1.x; x[5] = x1.y; x[6] = x1.z; x[7] = x1.w;
        if (!a.cross) {  // rotary (LGN:41-54,155): pair i of the lane <-> frequency 8s + 4 half + i
          const float* e = a.enc + ((size_t)item * a.nmax + qrow) * HD + 8 * s + 4 * half;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float c = e[i], sn = e[HF + i], t0 = x[2 * i], t1 = x[2 * i + 1];
            x[2 * i] = t0 * c + (-t1) * sn;
            x[2 * i + 1] = t1 * c + t0 * sn;
          }
        }
      }
      unsigned pc[4][NPL];
#pragma unroll
      for (int i = 0; i < 4; ++i) S::split(x[2 * i] * sc, x[2 * i + 1] * sc, S::act_scale(), pc[i]);
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) qf[s][pl] = u32x4{pc[0][pl], pc[1][pl], pc[2][pl], pc[3][pl]};
    }
  }
  f32x16 oacc[OBLK];
#pragma unroll
  for (int n = 0; n < OBLK; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[n][r] = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;

  // staging: NCP (6 / 9) straight 16-byte copies per thread per tile (images pre-built by kv_prep96_kernel)
  const u32x4* src = a.kv_img + (size_t)kitem * a.tiles * TILE_STRIDE96;
  auto load_tile = [&](int kt, int buf) {  // wave w moves slots w * 64 + 256 i + lane
    const u32x4* p = src + (size_t)(kt >> 5) * TILE_STRIDE96;
#pragma unroll
    for (int i = 0; i < NCP; ++i) lds_dma16(p + wv * 64 + 256 * i + lane, &img[buf * TILE_SLOTS + wv * 64 + 256 * i]);
  };
  // this workgroup's share of the key tiles (all of them unless the launcher split the key range)
  const int per = ((nk + 31) / 32 + a.splits - 1) / a.splits * 32;
  const int kt0 = sp * per, kt1 = min(nk, kt0 + per);
  if (kt0 < kt1) load_tile(kt0, 0);
  int buf = 0;
  for (int kt = kt0; kt < kt1; kt += 32, buf ^= 1) {
    // the compiler does not order the barrier after the DMA by itself; after it every wave has also left the tile that lived in the buffer
    // the next transfer overwrites
    lds_dma_wait_all();
    __syncthreads();
    if (kt + 32 < kt1) load_tile(kt + 32, buf ^ 1);
    const u32x4* Kp = img + buf * TILE_SLOTS;
    const u32x4* Vp = Kp + KSL;

    // ---- S^T = K · Q^T : 6 steps x cross terms ----
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < QSTEPS; ++s) {
      u32x4 kf[NPL];
#pragma unroll
      for (int p = 0; p < NPL; ++p) kf[p] = Kp[(p * KBLK + 2 * s + half) * 32 + lx];
#pragma unroll
      for (int tm = 0; tm < S::NT; ++tm) sacc = S::mma(kf[S::ta(tm)], qf[s][S::tb(tm)], sacc);
    }
    // fp16x3: sacc holds scale^2 x the scores; the exact power-of-two factor is applied inside the fused multiply-add of the exponent below

    // ---- online softmax (log2 domain, deferred rescale); the masked tail of the last key tile ----
    if (kt + 32 > nk) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kt + mfma_row(r, half) >= nk) sacc[r] = -INFINITY;
    }
    float tmax = fmaxf(fmaxf(sacc[0], sacc[1]), sacc[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) tmax = fmaxf(fmaxf(tmax, sacc[r]), sacc[r + 1]);
    tmax = fmaxf(tmax, sacc[15]);
    tmax = half_pair_max(tmax) * inv_qk;
    constexpr float RESCALE_LOG2 = 8.0f;
    if (__any(tmax > m_run + RESCALE_LOG2)) {
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int n = 0; n < OBLK; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[n][r] *= alpha;
      m_run = m_new;
    }
    const float p_shift = MODE == 2 ? 4.0f : 0.0f;  // log2(DIM_F16_ACT_SCALE): the probabilities come out already scaled for their split
    float p[16];
    float psum = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[r] = __builtin_amdgcn_exp2f(fmaf(sacc[r], inv_qk, p_shift - m_run));
      psum += p[r];
    }
    l_run += psum;

    // ---- O^T += V^T · P^T : registers 8u .. 8u + 7 of p are the B operand of step u ----
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      unsigned pc[4][NPL];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (MODE == 2) split2_pk_raw(p[8 * u + 2 * e], p[8 * u + 2 * e + 1], pc[e][0], pc[e][1]);
        else S::split(p[8 * u + 2 * e], p[8 * u + 2 * e + 1], S::act_scale(), pc[e]);
      }
      u32x4 pf[NPL];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) pf[pl] = u32x4{pc[0][pl], pc[1][pl], pc[2][pl], pc[3][pl]};
#pragma unroll
      for (int n = 0; n < OBLK; ++n) {
        u32x4 vf[NPL];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) vf[pl] = Vp[((pl * 2 + u) * 2 + half) * HD + n * 32 + lx];
#pragma unroll
        for (int tm = 0; tm < S::NT; ++tm) oacc[n] = S::mma(vf[S::ta(tm)], pf[S::tb(tm)], oacc[n]);
      }
    }
  }

  // fp16x3: the V·P accumulator holds scale^2 x the sum and l_run scale x the normaliser: divide by scale * l_run
  const float l_both = half_pair_sum(l_run);
  if (a.splits > 1) {  // partial result for attn_combine96_kernel
    if (qok) {
      float* pp = a.part + (((size_t)item * a.nmax + qrow) * a.splits + sp) * PART96;
#pragma unroll
      for (int n = 0; n < OBLK; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *(float4*)(pp + n * 32 + 8 * g + 4 * half) = make_float4(oacc[n][4 * g], oacc[n][4 * g + 1], oacc[n][4 * g + 2], oacc[n][4 * g + 3]);
      if (half == 0) { pp[HD] = m_run; pp[HD + 1] = l_both; }
    }
    return;
  }
  const float l_tot = l_both * (MODE == 2 ? S::act_scale() : 1.0f);
  if (qok) {
    float* op = a.o + (size_t)item * a.so + (size_t)qrow * a.ldo;
#pragma unroll
    for (int n = 0; n < OBLK; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);  // LGN:103-104: empty key set -> zeros
        if (nk > 0) o = make_float4(oacc[n][4 * g] / l_tot, oacc[n][4 * g + 1] / l_tot, oacc[n][4 * g + 2] / l_tot, oacc[n][4 * g + 3] / l_tot);
        *(float4*)(op + n * 32 + 8 * g + 4 * half) = o;
      }
  }
}

// merges the partial results of a split key range: 32 threads per query row, 24 of them with four output dims each
__global__ __launch_bounds__(256) void attn_combine96_kernel(AttnArgs96 a, float out_scale) {
  const int item = blockIdx.y, row = blockIdx.x * 8 + (threadIdx.x >> 5), d4 = (threadIdx.x & 31) * 4;
  if (a.done[item >> 1] != 0 || row >= a.n[item] || d4 >= HD) return;
  const float* pp = a.part + ((size_t)item * a.nmax + row) * a.splits * PART96;
  float M = -INFINITY, L = 0.f;
  float4 O = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < a.splits; ++s) M = fmaxf(M, pp[s * PART96 + HD]);
  for (int s = 0; s < a.splits; ++s) {
    const float ms = pp[s * PART96 + HD];
    const float w = (ms == -INFINITY) ? 0.f : exp2f(ms - M);
    const float4 os = *(const float4*)(pp + s * PART96 + d4);
    L += w * pp[s * PART96 + HD + 1];
    O.x += w * os.x; O.y += w * os.y; O.z += w * os.z; O.w += w * os.w;
  }
  const float den = L * out_scale;
  const float4 r = (L > 0.f) ? make_float4(O.x / den, O.y / den, O.z / den, O.w / den) : make_float4(0.f, 0.f, 0.f, 0.f);  // no keys -> zeros (LGN:103-104)
  *(float4*)(a.o + (size_t)item * a.so + (size_t)row * a.ldo + d4) = r;
}
}  // namespace

int launch_lgl_attention(const LgState& st, int cross, hipStream_t s) {
  const int mode = dim_precision_mode();
  DIM_REQUIRE(mode == 1 || mode == 2, "LighterGlue attention exists in the split arithmetics (fp16x3, bf16x6) only");
  DIM_REQUIRE(st.dim == 96 && st.heads == 1, "launch_lgl_attention: width %d / %d heads", st.dim, st.heads);
  AttnArgs96 a;
  const long long is = (long long)st.nmax * 288;
  if (!cross) { a.q = st.qkv; a.k = st.qkv + 96; a.v = st.qkv + 192; }
  else { a.q = st.qkv; a.k = st.qkv; a.v = st.qkv + 96; }
  a.ldq = a.ldk = a.ldv = 288; a.sq = a.sk = a.sv = is;
  a.o = st.ctx; a.ldo = 96; a.so = (long long)st.nmax * 96;
  a.n = st.n_cur; a.done = st.done; a.cross = cross;
  const float s4 = (float)pow((double)HD, -0.25), s2 = (float)pow((double)HD, -0.5);   // 96^-0.25, 96^-0.5 rounded once from fp64
  a.qscale = cross ? s4 : s2;
  a.kscale = cross ? s4 : 1.0f;
  a.sat = st.sat_qkv;
  a.enc = st.enc; a.kv_img = (u32x4*)st.kv_img; a.nmax = st.nmax; a.tiles = cdiv(st.nmax, 32);
  // small batches leave most CUs idle and make every workgroup walk all key tiles alone: cut the key range into the fewest parts (1, 2, 4)
  // that give the launch two workgroups per CU
  const int nsel = st.nsel > 0 ? st.nsel : st.nmax;
  const int wgs = cdiv(nsel, 128) * st.n_items;
  a.part = st.attn_part;
  a.splits = (st.attn_part && st.n_items <= st.attn_part_items) ? (wgs >= 512 ? 1 : (wgs >= 256 ? 2 : 4)) : 1;
  a.qblocks = cdiv(nsel, 128) * a.splits;
  a.groups = st.n_items;
  const dim3 grid((unsigned)(cdiv(a.groups, 8) * 8 * a.qblocks));  // whole rounds of 8 items, one per XCD (surplus workgroups exit)
  const dim3 pg(cdiv(nsel, 32), st.n_items);
  if (mode == 2) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(kv_prep96_kernel<2>), pg, dim3(256), 0, s, a);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_d96_kernel<2>), grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(kv_prep96_kernel<1>), pg, dim3(256), 0, s, a);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_d96_kernel<1>), grid, dim3(256), 0, s, a);
  }
  if (a.splits > 1) {
    const float out_scale = mode == 2 ? DIM_F16_ACT_SCALE : 1.0f;
    hipLaunchKernelGGL(attn_combine96_kernel, dim3(cdiv(nsel, 8), st.n_items), dim3(256), 0, s, a, out_scale);
  }
  DIM_LAUNCH_CHECK();
  return 0;
}
