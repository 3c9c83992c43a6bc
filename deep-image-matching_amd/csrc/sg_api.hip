// dim_sg_* : resident SuperGlue matcher (C ABI in include/dim_hip.h).  Replaces SuperGlue.forward (reference
// thirdparty/SuperGluePretrainedNetwork/models/superglue.py, SGN:250-305) as driven by matchers/superglue.py, batched over pairs.
//
// The attentional graph network is a composition of the LightGlue launchers on the 256-wide state of lg_handle.h's LgState (four heads of 64,
// scale 1/8): per layer one 256 -> 768 projection [q | k | v] (K | V tile images from its epilogue where the block shape allows), the
// split-precision attention (cross layers: keys / values of the other item; LgState::sg: no rotary, Q never from the K image), merge,
// mlp.0 on [x | message] with ReLU, mlp.3 with the residual.  BatchNorm is folded and the heads are permuted to head-major on the host
// (weights.py).  The encoder, Sinkhorn and the selection are sg_kernels.hip.
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/dim_hip.h"
#include "sg_kernels.h"

struct SgLayerW {
  SplitWeights qkv_x[3], merge_x[3], mlp0_x[3], mlp3_x[3];
  float *qkv_b, *merge_b, *mlp0_b, *mlp3_b;
};
struct dim_sg {
  DimHandleBase base;   // first member: dim_handle_tune_set
  int n_layers, max_pairs, nmax;
  int debug_layers = -1;   // dim_sg_debug_layers: parity taps stop the graph network after this many layers (-1 = all)
  std::vector<SgLayerW> L;
  float* enc_w[5]; float* enc_b[5];
  SplitWeights proj_x[3]; float* proj_b;
  LgState st;
  SgOt ot;
};

namespace {
int upload_x(DimHandleBase* hb, SplitWeights* dst, const std::vector<float>& w_kn, int K, int N) {
  for (int mode = 1; mode <= 2; ++mode)
    if (dim_upload_gemm_split(hb, &dst[mode], w_kn.data(), K, N, (N + 127) / 128 * 128, mode, 0) != 0) return -1;
  return 0;
}
// Conv1d(kernel 1) weight [out][in] -> GEMM operand [in][out], into columns [col0, col0 + out) of an operand `ld` wide
void put_t(std::vector<float>& dst, int ld, int col0, const float* w, int out_f, int in_f, float scale = 1.0f) {
  for (int o = 0; o < out_f; ++o)
    for (int i = 0; i < in_f; ++i) dst[(size_t)i * ld + col0 + o] = w[(size_t)o * in_f + i] * scale;
}
}  // namespace

extern "C" {

void dim_sg_destroy(dim_sg* h) {
  if (!h) return;
  dim_handle_release(&h->base);
  delete h;
}

int dim_sg_create(const dim_sg_weights* w, const dim_sg_config* cfg, int max_pairs, int max_kpts, dim_sg** out) {
  DIM_REQUIRE(w && cfg && out, "dim_sg_create: null argument");
  DIM_REQUIRE(cfg->descriptor_dim == 256, "dim_sg_create: descriptor_dim %d is not built (256: four heads of 64)", cfg->descriptor_dim);
  DIM_REQUIRE(cfg->n_layers > 0 && cfg->n_layers % 2 == 0 && cfg->n_layers <= 64,
              "dim_sg_create: n_layers %d must be a positive multiple of 2 (alternating self / cross), at most 64", cfg->n_layers);
  DIM_REQUIRE(w->layers && w->final_proj_w && w->final_proj_b, "dim_sg_create: null weights");
  DIM_REQUIRE(max_pairs > 0 && max_kpts > 0 && max_kpts <= 32768, "dim_sg_create: bad sizes (max_pairs %d, max_kpts %d)", max_pairs, max_kpts);
  DIM_REQUIRE(w->bin_score - w->bin_score == 0.0f, "dim_sg_create: bin_score is non-finite");
  for (int i = 0; i < 5; ++i) DIM_REQUIRE(w->kenc_w[i] && w->kenc_b[i], "dim_sg_create: keypoint encoder stage %d missing", i);
  std::unique_ptr<dim_sg, void (*)(dim_sg*)> guard(new dim_sg(), dim_sg_destroy);
  dim_sg* const h = guard.get();
  DimHandleBase* const hb = &h->base;
  h->n_layers = cfg->n_layers; h->max_pairs = max_pairs; h->nmax = (max_kpts + 3) & ~3;
  const int dims[6] = {3, 32, 64, 128, 256, 256};
  for (int i = 0; i < 5; ++i) {
    std::vector<float> t((size_t)dims[i] * dims[i + 1]);
    put_t(t, dims[i + 1], 0, w->kenc_w[i], dims[i + 1], dims[i]);
    DIM_TRY(dim_upload_f32(hb, &h->enc_w[i], t)); DIM_TRY(dim_upload_f32(hb, &h->enc_b[i], w->kenc_b[i], dims[i + 1]));
  }
  h->L.resize(cfg->n_layers);
  for (int i = 0; i < cfg->n_layers; ++i) {
    const dim_sg_layer_weights& s = w->layers[i];
    SgLayerW& d = h->L[i];
    DIM_REQUIRE(s.q_w && s.q_b && s.k_w && s.k_b && s.v_w && s.v_b && s.merge_w && s.merge_b && s.mlp0_w && s.mlp0_b && s.mlp3_w && s.mlp3_b,
                "dim_sg_create: layer %d: null weights", i);
    std::vector<float> qkv((size_t)256 * 768), qkvb(768);
    put_t(qkv, 768, 0, s.q_w, 256, 256); put_t(qkv, 768, 256, s.k_w, 256, 256); put_t(qkv, 768, 512, s.v_w, 256, 256);
    memcpy(&qkvb[0], s.q_b, 1024); memcpy(&qkvb[256], s.k_b, 1024); memcpy(&qkvb[512], s.v_b, 1024);
    DIM_TRY(upload_x(hb, d.qkv_x, qkv, 256, 768)); DIM_TRY(dim_upload_f32(hb, &d.qkv_b, qkvb));
    std::vector<float> t((size_t)256 * 256);
    put_t(t, 256, 0, s.merge_w, 256, 256);
    DIM_TRY(upload_x(hb, d.merge_x, t, 256, 256)); DIM_TRY(dim_upload_f32(hb, &d.merge_b, s.merge_b, 256));
    t.assign((size_t)512 * 512, 0.0f);
    put_t(t, 512, 0, s.mlp0_w, 512, 512);
    DIM_TRY(upload_x(hb, d.mlp0_x, t, 512, 512)); DIM_TRY(dim_upload_f32(hb, &d.mlp0_b, s.mlp0_b, 512));
    t.assign((size_t)512 * 256, 0.0f);
    put_t(t, 256, 0, s.mlp3_w, 256, 512);
    DIM_TRY(upload_x(hb, d.mlp3_x, t, 512, 256)); DIM_TRY(dim_upload_f32(hb, &d.mlp3_b, s.mlp3_b, 256));
  }
  {  // final_proj / 4 on both sides = scores / 16 = / 256^0.5 (SGN:279-280): a power of two, folding it is exact
    std::vector<float> t((size_t)256 * 256), b(256);
    put_t(t, 256, 0, w->final_proj_w, 256, 256, 0.25f);
    for (int i = 0; i < 256; ++i) b[i] = w->final_proj_b[i] * 0.25f;
    DIM_TRY(upload_x(hb, h->proj_x, t, 256, 256)); DIM_TRY(dim_upload_f32(hb, &h->proj_b, b));
  }
  LgState& st = h->st;
  memset(&st, 0, sizeof(st));
  const size_t P = max_pairs, I = 2 * P, N = h->nmax;
  st.dim = 256; st.heads = 4; st.head_dim = 64; st.sg = 1;
  st.n_pairs = max_pairs; st.n_items = 2 * max_pairs; st.nmax = h->nmax; st.nsel = h->nmax;
  DIM_TRY(dim_dev_alloc(hb, &st.desc, I * N * 256)); DIM_TRY(dim_dev_alloc(hb, &st.qkv, I * N * 768));
  DIM_TRY(dim_dev_alloc(hb, &st.ctx, I * N * 256)); DIM_TRY(dim_dev_alloc(hb, &st.msg, I * N * 256));
  DIM_TRY(dim_dev_alloc(hb, &st.hid, I * N * 512)); DIM_TRY(dim_dev_alloc(hb, &st.md, I * N * 256));
  DIM_TRY(dim_dev_alloc(hb, &st.sim, P * N * N));
  DIM_TRY(dim_dev_alloc(hb, &st.n_cur, I)); DIM_TRY(dim_dev_alloc(hb, &st.done, P));
  { unsigned char* kvp = nullptr; DIM_TRY(dim_dev_alloc(hb, &kvp, I * 4 * ((N + 31) / 32) * 1536 * 16)); st.kv_img = kvp; }
  // no key-split scratch: launch_lg_attention_x6 then never cuts the key range, so a pair's attention sums in ONE order whether it runs alone
  // or in a batch (the split's partial records merge in another order; LightGlue accepts that, SuperGlue's tests ask batch = singles bit for bit)
  st.attn_part = nullptr; st.attn_part_items = 0;
  SgOt& ot = h->ot;
  ot.alpha = w->bin_score;
  DIM_TRY(dim_dev_alloc(hb, &ot.u, P * (N + 1))); DIM_TRY(dim_dev_alloc(hb, &ot.v, P * (N + 1)));
  DIM_TRY(dim_dev_alloc(hb, &ot.arg0, P * N)); DIM_TRY(dim_dev_alloc(hb, &ot.arg1, P * N)); DIM_TRY(dim_dev_alloc(hb, &ot.val0, P * N));
  *out = guard.release();
  return 0;
}

int dim_sg_max_kpts(dim_sg* h) { return h ? h->nmax : -1; }

int dim_sg_match(dim_sg* h, const float* kpts_tab_dev, const float* desc_tab_dev, const float* score_tab_dev, const int32_t* n_tab_dev,
                 const float* size_tab_dev, int cap, const int32_t* pair_idx_dev, int n_pairs, int sinkhorn_iterations, float match_threshold,
                 int64_t* matches_dev, float* mscores_dev, int32_t* n_matches_dev, int32_t* matches01_dev, float* mscores01_dev, void* stream) {
  DIM_REQUIRE(h && kpts_tab_dev && desc_tab_dev && score_tab_dev && n_tab_dev && size_tab_dev, "dim_sg_match: null input");
  DimTuneScope tune_scope(&h->base);
  DIM_REQUIRE(matches_dev && mscores_dev && n_matches_dev && matches01_dev && mscores01_dev, "dim_sg_match: null output");
  DIM_REQUIRE(n_pairs >= 1 && n_pairs <= h->max_pairs, "dim_sg_match: n_pairs %d outside [1,%d]", n_pairs, h->max_pairs);
  DIM_REQUIRE(cap > 0, "dim_sg_match: cap");
  DIM_REQUIRE(sinkhorn_iterations >= 0, "dim_sg_match: sinkhorn_iterations %d is negative", sinkhorn_iterations);
  const int pmode = dim_precision_mode();
  DIM_REQUIRE(pmode == 1 || pmode == 2, "dim_sg_match: SuperGlue runs in the split arithmetics (fp16x3, bf16x6) only, not fp32");
  hipStream_t s = (hipStream_t)stream;
  LgState st = h->st;
  st.n_pairs = n_pairs; st.n_items = 2 * n_pairs;
  const int N = st.nmax, I = st.n_items;
  const int Nsel = std::min(N, (cap + 3) & ~3);   // launch shapes follow the table's rows per image, strides follow N (dim_lg_match)
  st.nsel = Nsel;
  const long long s256 = (long long)N * 256, s512 = (long long)N * 512, s768 = (long long)N * 768;
  // fp16x3 range guard (dim_common.h).  SuperGlue has no LayerNorm: nothing bounds the residual stream, every producer of a split operand reports
  auto sat = [&](int site) -> unsigned* { return pmode == 2 ? dim_sat_counter(site) : nullptr; };
  st.sat_qkv = sat(DIM_SAT_LG_QKV); st.sat_ffn = sat(DIM_SAT_LG_FFN);
  SgEncW ew;
  for (int i = 0; i < 5; ++i) { ew.w[i] = h->enc_w[i]; ew.b[i] = h->enc_b[i]; }
  DIM_RUN(launch_sg_encoder(st, ew, kpts_tab_dev, desc_tab_dev, score_tab_dev, n_tab_dev, size_tab_dev, pair_idx_dev, cap, sat(DIM_SAT_LG_INPUT), s));
  auto gemm_items = [&](const float* A, int lda, long long sA, const float* A1, int lda1, long long sA1, int ksplit, const SplitWeights* Bx,
                        const float* bias, const float* R, float* C, int ldc, long long sC, int Nn, int K, int relu, unsigned* sat_ctr) -> int {
    GemmArgs g;
    g.A0 = A; g.lda0 = lda; g.strideA0 = sA; g.A1 = A1; g.lda1 = lda1; g.strideA1 = sA1; g.ksplit = ksplit;
    g.bias = bias; g.R = R; g.ldr = ldc; g.strideR = sC; g.C = C; g.ldc = ldc; g.strideC = sC;
    g.M = Nsel; g.N = Nn; g.K = K; g.rows = st.n_cur; g.flag = st.done; g.flag_shift = 1; g.flag_eq = 0;
    g.relu = relu; g.sat = sat_ctr;
    g.set_split(Bx[pmode]);
    return launch_gemm_x6(g, I, s);
  };
  const bool fuse_kv = pmode == 2 && dim_fuse_kv() && gemm_x6_fuses_kv(Nsel, 768, I, 2);
  const int Lr = h->debug_layers >= 0 ? std::min(h->debug_layers, h->n_layers) : h->n_layers;
  for (int i = 0; i < Lr; ++i) {
    const SgLayerW& w = h->L[i];
    const int cross = i & 1;   // GNN_layers = ["self", "cross"] * (n_layers / 2) (SGN:216)
    // q | k | v of every item from its own descriptors; a cross layer's attention reads the OTHER item's k and v (SGN:143-147)
    if (fuse_kv) {
      GemmArgs g;
      g.A0 = st.desc; g.lda0 = 256; g.strideA0 = s256; g.bias = w.qkv_b; g.C = st.qkv; g.ldc = 768; g.strideC = s768;
      g.M = Nsel; g.N = 768; g.K = 256; g.rows = st.n_cur; g.flag = st.done; g.flag_shift = 1; g.flag_eq = 0; g.sat = st.sat_qkv;
      g.kv_img = st.kv_img; g.kv_tiles = (N + 31) / 32; g.kv_kblock = 1; g.kv_vblock = 2; g.kv_nmax = N; g.kv_enc = nullptr;
      g.set_split(w.qkv_x[2]);
      DIM_RUN(launch_gemm_x6(g, I, s));
    } else {
      DIM_RUN(gemm_items(st.desc, 256, s256, nullptr, 0, 0, 0, w.qkv_x, w.qkv_b, nullptr, st.qkv, 768, s768, 768, 256, 0, st.sat_qkv));
    }
    dim_prof_begin(cross ? DIM_PROF_LG_CROSS_ATTN : DIM_PROF_LG_SELF_ATTN, s);
    DIM_RUN(launch_lg_attention_x6(st, cross, s, fuse_kv ? 1 : 0));
    dim_prof_end(cross ? DIM_PROF_LG_CROSS_ATTN : DIM_PROF_LG_SELF_ATTN, s);
    DIM_RUN(gemm_items(st.ctx, 256, s256, nullptr, 0, 0, 0, w.merge_x, w.merge_b, nullptr, st.msg, 256, s256, 256, 256, 0, st.sat_ffn));
    DIM_RUN(gemm_items(st.desc, 256, s256, st.msg, 256, s256, 256, w.mlp0_x, w.mlp0_b, nullptr, st.hid, 512, s512, 512, 512, 1, st.sat_ffn));
    DIM_RUN(gemm_items(st.hid, 512, s512, nullptr, 0, 0, 0, w.mlp3_x, w.mlp3_b, st.desc, st.desc, 256, s256, 256, 512, 0, sat(DIM_SAT_LG_DESC)));
  }
  DIM_RUN(gemm_items(st.desc, 256, s256, nullptr, 0, 0, 0, h->proj_x, h->proj_b, nullptr, st.md, 256, s256, 256, 256, 0, sat(DIM_SAT_LG_DESC)));
  {
    GemmArgs g;
    g.A0 = st.md; g.lda0 = 256; g.strideA0 = 2 * s256; g.B = st.md + s256; g.ldb = 256; g.strideB = 2 * s256; g.bt = 1;
    g.C = st.sim; g.ldc = N; g.strideC = (long long)N * N; g.M = Nsel; g.N = Nsel; g.K = 256;
    g.rows = st.n_cur; g.rows_mul = 2; g.rows_off = 0; g.cols = st.n_cur; g.cols_mul = 2; g.cols_off = 1;
    g.flag = st.done; g.flag_shift = 0; g.flag_eq = 0;
    DIM_RUN(launch_gemm_x6_nt(g, n_pairs, pmode, s));
  }
  DIM_RUN(dim_sg_sinkhorn(h, n_pairs, cap, sinkhorn_iterations, stream));
  return launch_sg_select(st, h->ot, match_threshold, N, (long long*)matches_dev, mscores_dev, n_matches_dev, matches01_dev, mscores01_dev, s);
}

int dim_sg_sinkhorn(dim_sg* h, int n_pairs, int cap, int sinkhorn_iterations, void* stream) {
  DIM_REQUIRE(h, "dim_sg_sinkhorn: null handle");
  DIM_REQUIRE(n_pairs >= 1 && n_pairs <= h->max_pairs && cap > 0, "dim_sg_sinkhorn: n_pairs %d outside [1,%d] or cap %d", n_pairs, h->max_pairs, cap);
  DIM_REQUIRE(sinkhorn_iterations >= 0, "dim_sg_sinkhorn: sinkhorn_iterations %d is negative", sinkhorn_iterations);
  hipStream_t s = (hipStream_t)stream;
  LgState st = h->st;
  st.n_pairs = n_pairs; st.n_items = 2 * n_pairs;
  st.nsel = std::min(st.nmax, (cap + 3) & ~3);
  const size_t uv = (size_t)n_pairs * (st.nmax + 1) * sizeof(float);
  DIM_HIP(hipMemsetAsync(h->ot.u, 0, uv, s)); DIM_HIP(hipMemsetAsync(h->ot.v, 0, uv, s));   // u = v = 0 (SGN:156)
  for (int it = 0; it < sinkhorn_iterations; ++it) {
    DIM_RUN(launch_sg_sinkhorn_rows(st, h->ot, s));
    DIM_RUN(launch_sg_sinkhorn_cols(st, h->ot, s));
  }
  return 0;
}

int dim_sg_select(dim_sg* h, int n_pairs, int cap, float match_threshold, int64_t* matches_dev, float* mscores_dev, int32_t* n_matches_dev,
                  int32_t* matches01_dev, float* mscores01_dev, void* stream) {
  DIM_REQUIRE(h && matches_dev && mscores_dev && n_matches_dev && matches01_dev && mscores01_dev, "dim_sg_select: null argument");
  DIM_REQUIRE(n_pairs >= 1 && n_pairs <= h->max_pairs && cap > 0, "dim_sg_select: n_pairs %d outside [1,%d] or cap %d", n_pairs, h->max_pairs, cap);
  LgState st = h->st;
  st.n_pairs = n_pairs; st.n_items = 2 * n_pairs;
  st.nsel = std::min(st.nmax, (cap + 3) & ~3);
  return launch_sg_select(st, h->ot, match_threshold, st.nmax, (long long*)matches_dev, mscores_dev, n_matches_dev, matches01_dev, mscores01_dev,
                          (hipStream_t)stream);
}

int dim_sg_debug_layers(dim_sg* h, int n_layers) {
  DIM_REQUIRE(h, "dim_sg_debug_layers: null handle");
  h->debug_layers = n_layers;
  return 0;
}

int dim_sg_debug(dim_sg* h, float** desc, float** scores, float** u, float** v, int32_t** n_cur, int32_t** done) {
  DIM_REQUIRE(h, "dim_sg_debug: null handle");
  if (desc) *desc = h->st.desc;
  if (scores) *scores = h->st.sim;
  if (u) *u = h->ot.u;
  if (v) *v = h->ot.v;
  if (n_cur) *n_cur = h->st.n_cur;
  if (done) *done = h->st.done;
  return 0;
}

}  // extern "C"
