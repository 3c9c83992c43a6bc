// dim_lgl_create: LighterGlue, the matcher XFeat was trained with — LightGlue (LGN) at input_dim 64, descriptor_dim 96, ONE head of 96,
// 6 layers (reference thirdparty/accelerated_features/modules/lighterglue.py:12-27).  The handle is an ordinary dim_lg: dim_lg_match
// (lg_api.hip) hands a call on it to lgl_match below, which enqueues the same forward on the 96-wide kernels (lg_attn_d96.hip,
// lgl_kernels.hip) and on gemm_x6.hip's split GEMM through its n_pad path (N = 96 / 192 / 288 inside 128 / 256 / 384 padded columns).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "lg_handle.h"

namespace {
constexpr int D = 96, D2 = 192, D3 = 288;

int upload_x(DimHandleBase* hb, SplitWeights* dst, const std::vector<float>& w_kn, int K, int N) {
  for (int mode = 1; mode <= 2; ++mode)
    if (dim_upload_gemm_split(hb, &dst[mode], w_kn.data(), K, N, (N + 127) / 128 * 128, mode, 0) != 0) return -1;
  return 0;
}
// nn.Linear weight [out][in] -> GEMM operand [in][out]
std::vector<float> transpose(const float* w, int out_f, int in_f) {
  std::vector<float> t((size_t)in_f * out_f);
  for (int o = 0; o < out_f; ++o)
    for (int i = 0; i < in_f; ++i) t[(size_t)i * out_f + o] = w[(size_t)o * in_f + i];
  return t;
}
int linear(DimHandleBase* hb, SplitWeights* wx, float** bias, const float* w, const float* b, int out_f, int in_f) {
  if (upload_x(hb, wx, transpose(w, out_f, in_f), in_f, out_f) != 0) return -1;
  return dim_upload_f32(hb, bias, b, out_f);
}
}  // namespace

extern "C" int dim_lgl_create(const dim_lg_weights* w, const dim_lg_config* cfg, int descriptor_dim, int num_heads, int max_pairs, int max_kpts,
                              dim_lg** out) {
  DIM_REQUIRE(w && cfg && out && w->layers, "dim_lgl_create: null argument");
  if (descriptor_dim == 256 && num_heads == 4) return dim_lg_create(w, cfg, max_pairs, max_kpts, out);
  DIM_REQUIRE(descriptor_dim == D && num_heads == 1, "dim_lgl_create: descriptor_dim %d with %d heads is not built (96 with 1 head, or 256 with 4)",
              descriptor_dim, num_heads);
  DIM_REQUIRE(w->n_layers >= 1 && w->n_layers <= 32, "dim_lgl_create: n_layers %d", w->n_layers);
  DIM_REQUIRE(w->input_dim > 0 && w->input_dim % 32 == 0, "dim_lgl_create: input_dim %d must be a multiple of 32", w->input_dim);
  DIM_REQUIRE(w->input_proj_w && w->input_proj_b, "dim_lgl_create: input_proj is required (the feature table is projected to width 96 on the device)");
  DIM_REQUIRE(w->posenc_Wr && w->confidence_thresholds, "dim_lgl_create: null weights");
  DIM_REQUIRE(max_pairs > 0 && max_kpts > 0, "dim_lgl_create: bad sizes");
  std::unique_ptr<dim_lg, void (*)(dim_lg*)> guard(new dim_lg(), dim_lg_destroy);
  dim_lg* const h = guard.get();
  DimHandleBase* const hb = &h->base;
  h->cfg = *cfg;
  h->n_layers = w->n_layers; h->input_dim = w->input_dim; h->max_pairs = max_pairs;
  h->nmax = (max_kpts + 3) & ~3;
  h->inproj_w = h->inproj_b = nullptr;
  h->thr.assign(w->confidence_thresholds, w->confidence_thresholds + w->n_layers);
  DIM_TRY(dim_upload_f32(hb, &h->Wr, w->posenc_Wr, D));   // (head_dim / 2, 2)
  DIM_TRY(dim_upload_f32(hb, &h->inproj_w, transpose(w->input_proj_w, D, w->input_dim)));
  DIM_TRY(dim_upload_f32(hb, &h->inproj_b, w->input_proj_b, D));
  h->L.resize(w->n_layers);
  for (int i = 0; i < w->n_layers; ++i) {
    const dim_lg_layer_weights& s = w->layers[i];
    LayerW& d = h->L[i];   // (value-initialised: the fp32 operand copies of the 256-wide path's fp32 mode stay null)
    // Wqkv rows are interleaved dim * 3 + {q, k, v} (LGN:153-154, one head); emit columns [q | k | v]
    std::vector<float> qkv((size_t)D * D3), qkvb(D3);
    for (int which = 0; which < 3; ++which)
      for (int dd = 0; dd < D; ++dd) {
        const int o = dd * 3 + which, c = which * D + dd;
        qkvb[c] = s.self_Wqkv_b[o];
        for (int k = 0; k < D; ++k) qkv[(size_t)k * D3 + c] = s.self_Wqkv_w[(size_t)o * D + k];
      }
    DIM_TRY(upload_x(hb, d.qkv_x, qkv, D, D3)); DIM_TRY(dim_upload_f32(hb, &d.qkv_b, qkvb));
    DIM_TRY(linear(hb, d.out_x, &d.out_b, s.self_out_w, s.self_out_b, D, D));
    DIM_TRY(linear(hb, d.sffn0_x, &d.sffn0_b, s.self_ffn0_w, s.self_ffn0_b, D2, D2));
    DIM_TRY(dim_upload_f32(hb, &d.sln_w, s.self_ln_w, D2)); DIM_TRY(dim_upload_f32(hb, &d.sln_b, s.self_ln_b, D2));
    DIM_TRY(linear(hb, d.sffn3_x, &d.sffn3_b, s.self_ffn3_w, s.self_ffn3_b, D, D2));
    // to_qk and to_v fused into one [96][192] operand: columns [qk | v]
    std::vector<float> cq((size_t)D * D2), cqb(D2);
    for (int o = 0; o < D; ++o) {
      cqb[o] = s.cross_qk_b[o]; cqb[D + o] = s.cross_v_b[o];
      for (int k = 0; k < D; ++k) {
        cq[(size_t)k * D2 + o] = s.cross_qk_w[(size_t)o * D + k];
        cq[(size_t)k * D2 + D + o] = s.cross_v_w[(size_t)o * D + k];
      }
    }
    DIM_TRY(upload_x(hb, d.cqkv_x, cq, D, D2)); DIM_TRY(dim_upload_f32(hb, &d.cqkv_b, cqb));
    DIM_TRY(linear(hb, d.cout_x, &d.cout_b, s.cross_out_w, s.cross_out_b, D, D));
    DIM_TRY(linear(hb, d.cffn0_x, &d.cffn0_b, s.cross_ffn0_w, s.cross_ffn0_b, D2, D2));
    DIM_TRY(dim_upload_f32(hb, &d.cln_w, s.cross_ln_w, D2)); DIM_TRY(dim_upload_f32(hb, &d.cln_b, s.cross_ln_b, D2));
    DIM_TRY(linear(hb, d.cffn3_x, &d.cffn3_b, s.cross_ffn3_w, s.cross_ffn3_b, D, D2));
    DIM_TRY(dim_upload_f32(hb, &d.match_w, s.assign_match_w, D)); DIM_TRY(dim_upload_f32(hb, &d.match_b, s.assign_match_b, 1));
    // final_proj as it is: the division by 96^0.25 is lgl_scale_md_kernel's (no power of two: folding it would round every weight)
    DIM_TRY(linear(hb, d.proj_x, &d.proj_b, s.assign_proj_w, s.assign_proj_b, D, D));
    if (s.token_w) { DIM_TRY(dim_upload_f32(hb, &d.tok_w, s.token_w, D)); DIM_TRY(dim_upload_f32(hb, &d.tok_b, s.token_b, 1)); }
    DIM_REQUIRE(i == w->n_layers - 1 || s.token_w, "dim_lgl_create: token_confidence.%d missing", i);
  }
  LgState& st = h->st;
  const size_t P = max_pairs, I = 2 * P, N = h->nmax;
  st.dim = D; st.heads = 1; st.head_dim = D;
  st.n_pairs = max_pairs; st.n_items = 2 * max_pairs; st.nmax = h->nmax; st.nsel = h->nmax;
  st.msg = nullptr;
  DIM_TRY(dim_dev_alloc(hb, &st.desc, I * N * D)); DIM_TRY(dim_dev_alloc(hb, &st.enc, I * N * D));
  DIM_TRY(dim_dev_alloc(hb, &st.qkv, I * N * D3)); DIM_TRY(dim_dev_alloc(hb, &st.ctx, I * N * D));
  DIM_TRY(dim_dev_alloc(hb, &st.msg, I * N * D)); DIM_TRY(dim_dev_alloc(hb, &st.hid, I * N * D2));
  DIM_TRY(dim_dev_alloc(hb, &st.md, I * N * D)); DIM_TRY(dim_dev_alloc(hb, &st.sim, P * N * N));
  DIM_TRY(dim_dev_alloc(hb, &st.conf, I * N)); DIM_TRY(dim_dev_alloc(hb, &st.mtch, I * N)); DIM_TRY(dim_dev_alloc(hb, &st.zls, I * N));
  DIM_TRY(dim_dev_alloc(hb, &st.rmax, I * N)); DIM_TRY(dim_dev_alloc(hb, &st.rlse, I * N)); DIM_TRY(dim_dev_alloc(hb, &st.best, I * N));
  DIM_TRY(dim_dev_alloc(hb, &st.arg, I * N)); DIM_TRY(dim_dev_alloc(hb, &st.n_cur, I)); DIM_TRY(dim_dev_alloc(hb, &st.n_new, I));
  DIM_TRY(dim_dev_alloc(hb, &st.n_orig, I)); DIM_TRY(dim_dev_alloc(hb, &st.ind, I * N)); DIM_TRY(dim_dev_alloc(hb, &st.dest, I * N));
  DIM_TRY(dim_dev_alloc(hb, &st.prune, I * N)); DIM_TRY(dim_dev_alloc(hb, &st.done, P)); DIM_TRY(dim_dev_alloc(hb, &st.cnt_lt, P));
  { unsigned char* kvp = nullptr; DIM_TRY(dim_dev_alloc(hb, &kvp, I * ((N + 31) / 32) * 2304 * 16)); st.kv_img = kvp; }
  st.attn_part_items = (int)(I < 8 ? I : 8);  // key-split attention only pays for <= 4 pairs
  DIM_TRY(dim_dev_alloc(hb, &st.attn_part, (size_t)st.attn_part_items * N * 4 * 100));
  DIM_TRY(dim_dev_alloc(hb, &st.tdesc, I * N * D)); DIM_TRY(dim_dev_alloc(hb, &st.tenc, I * N * D)); DIM_TRY(dim_dev_alloc(hb, &st.tind, I * N));
  *out = guard.release();
  return 0;
}

int lgl_match(dim_lg* h, const float* kpts_tab_dev, const float* desc_tab_dev, const int32_t* n_tab_dev, const float* size_tab_dev, int cap,
              const int32_t* pair_idx_dev, int n_pairs, int64_t* matches_dev, float* mscores_dev, int32_t* n_matches_dev, int32_t* matches01_dev,
              float* mscores01_dev, int32_t* stop_dev, int32_t* prune01_dev, float* dense_scores_dev, hipStream_t s) {
  const int pmode = dim_precision_mode();
  DIM_REQUIRE(pmode == 1 || pmode == 2, "dim_lg_match: a 96-wide handle runs in the split arithmetics (fp16x3, bf16x6) only, not fp32");
  LgState st = h->st;
  st.n_pairs = n_pairs; st.n_items = 2 * n_pairs;
  const int N = st.nmax, I = st.n_items, Lr = h->n_layers;
  const int Nsel = std::min(N, (cap + 3) & ~3);   // launch shapes follow the table's rows per image, strides follow N (dim_lg_match)
  st.nsel = Nsel;
  const long long s96 = (long long)N * D, s192 = (long long)N * D2, s288 = (long long)N * D3;
  const bool early = h->cfg.depth_confidence > 0, prune = h->cfg.width_confidence > 0;  // LGN:480-481
  // fp16x3 range guard (dim_common.h): the sites of the 256-wide path, fed by the same producers
  auto sat = [&](int site) -> unsigned* { return pmode == 2 ? dim_sat_counter(site) : nullptr; };
  st.sat_qkv = sat(DIM_SAT_LG_QKV); st.sat_ffn = sat(DIM_SAT_LG_FFN);
  DIM_RUN(launch_lgl_init(st, kpts_tab_dev, n_tab_dev, size_tab_dev, pair_idx_dev, cap, h->Wr, s));
  {  // input_proj (LGN:473-474) straight from the feature table
    GemmArgs g;
    g.A0 = desc_tab_dev; g.lda0 = h->input_dim; g.strideA0 = (long long)cap * h->input_dim; g.a_idx = pair_idx_dev;
    g.B = h->inproj_w; g.ldb = D; g.bias = h->inproj_b; g.C = st.desc; g.ldc = D; g.strideC = s96;
    g.M = Nsel; g.N = D; g.K = h->input_dim; g.rows = st.n_cur; g.sat = sat(DIM_SAT_LG_INPUT);
    DIM_RUN(launch_gemm(g, I, s));
  }
  // C[item] = [A | A1] * W + bias (+ R) over the live rows of the items whose pair is still iterating
  auto gemm_items = [&](const float* A, int lda, long long sA, const float* A1, int lda1, long long sA1, int ksplit, const SplitWeights* Bx,
                        const float* bias, const float* R, float* C, int ldc, long long sC, int Nn, int K, int flag_eq, unsigned* sat_ctr) -> int {
    GemmArgs g;
    g.A0 = A; g.lda0 = lda; g.strideA0 = sA; g.A1 = A1; g.lda1 = lda1; g.strideA1 = sA1; g.ksplit = ksplit;
    g.bias = bias; g.R = R; g.ldr = ldc; g.strideR = sC; g.C = C; g.ldc = ldc; g.strideC = sC;
    g.M = Nsel; g.N = Nn; g.K = K; g.rows = st.n_cur; g.flag = st.done; g.flag_shift = 1; g.flag_eq = flag_eq;
    g.sat = sat_ctr;
    g.set_split(Bx[pmode]);
    return launch_gemm_x6(g, I, s);
  };
  // out_proj / to_out, ffn.0 on [desc | message], LayerNorm + GELU, ffn.3 + residual (LGN:139-144,159,209)
  auto feed_forward = [&](const SplitWeights* out_x, const float* out_b, const SplitWeights* f0_x, const float* f0_b, const float* ln_w, const float* ln_b,
                          const SplitWeights* f3_x, const float* f3_b) -> int {
    DIM_RUN(gemm_items(st.ctx, D, s96, nullptr, 0, 0, 0, out_x, out_b, nullptr, st.msg, D, s96, D, D, 0, nullptr));
    DIM_RUN(gemm_items(st.desc, D, s96, st.msg, D, s96, D, f0_x, f0_b, nullptr, st.hid, D2, s192, D2, D2, 0, nullptr));
    DIM_RUN(launch_lgl_ln_gelu(st, ln_w, ln_b, s));
    return gemm_items(st.hid, D2, s192, nullptr, 0, 0, 0, f3_x, f3_b, st.desc, st.desc, D, s96, D, D2, 0, sat(DIM_SAT_LG_DESC));
  };
  // assignment (LGN:540-542) for the pairs that stopped at layer tag - 1, with its weights
  auto assignment = [&](int tag, const LayerW& w) -> int {
    DIM_RUN(gemm_items(st.desc, D, s96, nullptr, 0, 0, 0, w.proj_x, w.proj_b, nullptr, st.md, D, s96, D, D, tag, nullptr));
    DIM_RUN(launch_lgl_scale_md(st, tag, sat(DIM_SAT_LG_DESC), s));   // guarded: the similarity splits it
    GemmArgs g;
    g.A0 = st.md; g.lda0 = D; g.strideA0 = 2 * s96; g.B = st.md + s96; g.ldb = D; g.strideB = 2 * s96; g.bt = 1;
    g.C = st.sim; g.ldc = N; g.strideC = (long long)N * N; g.M = Nsel; g.N = Nsel; g.K = D;
    g.rows = st.n_cur; g.rows_mul = 2; g.rows_off = 0; g.cols = st.n_cur; g.cols_mul = 2; g.cols_off = 1;
    g.flag = st.done; g.flag_shift = 0; g.flag_eq = tag;
    DIM_RUN(launch_gemm_x6_nt(g, n_pairs, pmode, s));
    DIM_RUN(launch_lg_assign_stats(st, tag, w.match_w, w.match_b, s));
    return launch_lg_assign_argmax(st, tag, dense_scores_dev, s);
  };
  for (int i = 0; i < Lr; ++i) {
    const LayerW& w = h->L[i];
    // ---- self block (LGN:146-159) ----
    DIM_RUN(gemm_items(st.desc, D, s96, nullptr, 0, 0, 0, w.qkv_x, w.qkv_b, nullptr, st.qkv, D3, s288, D3, D, 0, st.sat_qkv));
    dim_prof_begin(DIM_PROF_LG_SELF_ATTN, s);
    DIM_RUN(launch_lgl_attention(st, 0, s));
    dim_prof_end(DIM_PROF_LG_SELF_ATTN, s);
    DIM_RUN(feed_forward(w.out_x, w.out_b, w.sffn0_x, w.sffn0_b, w.sln_w, w.sln_b, w.sffn3_x, w.sffn3_b));
    // ---- cross block (LGN:186-211) ----
    DIM_RUN(gemm_items(st.desc, D, s96, nullptr, 0, 0, 0, w.cqkv_x, w.cqkv_b, nullptr, st.qkv, D3, s288, D2, D, 0, st.sat_qkv));
    dim_prof_begin(DIM_PROF_LG_CROSS_ATTN, s);
    DIM_RUN(launch_lgl_attention(st, 1, s));
    dim_prof_end(DIM_PROF_LG_CROSS_ATTN, s);
    DIM_RUN(feed_forward(w.cout_x, w.cout_b, w.cffn0_x, w.cffn0_b, w.cln_w, w.cln_b, w.cffn3_x, w.cffn3_b));
    // ---- adaptive depth / width (LGN:494-516) ----
    const bool last = (i == Lr - 1);
    if (!last && (early || prune)) DIM_RUN(launch_lgl_confidence(st, w.tok_w, w.tok_b, w.match_w, w.match_b, h->thr[i], early ? 1 : 0, s));
    if (last || early) DIM_RUN(launch_lg_decide(st, i, (float)h->cfg.depth_confidence, early ? 1 : 0, last ? 1 : 0, s));
    if (last || early) DIM_RUN(assignment(i + 1, w));
    if (!last && prune) DIM_RUN(launch_lg_prune(st, i, h->cfg.width_confidence, h->thr[i], early ? 1 : 0, h->cfg.pruning_min_kpts, s));
  }
  DIM_RUN(launch_lg_finalize(st, Lr, prune ? 1 : 0, (float)h->cfg.filter_threshold, N, (long long*)matches_dev, mscores_dev, n_matches_dev,
                            matches01_dev, mscores01_dev, stop_dev, prune01_dev, s));
  return 0;
}
