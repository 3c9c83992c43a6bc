// dim_alike_* : resident ALIKE extractor (C ABI in include/dim_hip.h).
// Replaces ALike.__init__ / extract_dense_map / forward (thirdparty/alike/alike.py:59-179 = AKM) over ALNet (alnet.py:87-183 = AKN) and DKD
// (soft_detect.py:74-234 = AKD) as driven by AlikeExtractor (extractors/alike.py:22-44): sub_pixel=True, top_k / scores_th / n_limit from the config.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/dim_hip.h"
#include "alike_kernels.h"
#include "aliked_kernels.h"
#include "nhwc_conv.h"
#include "sp_kernels.h"

namespace {
constexpr int AK_BAND_PIXELS = 16384;   // alike-l's score map: pixels per row band of the convhead1 product (scratch independent of the image height)
}  // namespace

struct dim_alike {
  DimHandleBase base;   // first member: dim_handle_tune_set
  dim_alike_config cfg;
  int max_batch, max_h, max_w, capacity, stride;
  NhwcConvLayer L[8], A[3];   // the eight 3x3 convolutions (the ResBlock tails carry their downsample: the BatchNorm scale is folded into the 3x3 rows only), conv2 / conv3 / conv4
  float *w1, *ws, *h1_w, *h2_w;   // conv1 [c1p][q]; score row of convhead2 [dim]; convhead1 / convhead2[0:dim] as [dim][dim] GEMM operands
  SplitWeights g_h1, g_h2;
  float *t1, *x1, *p2, *t2, *x2, *p3, *t3, *x3, *p4, *t4, *x4, *f2, *f3, *f4, *q2, *q3, *q4, *score, *nms;
  float *X, *Y;   // head scratch: rows of x1234 and of the head products ([batch][rows_cap][dim])
  size_t rows_cap;
  float *cand_score, *kpts_px, *sc_tmp, *kpts_norm, *disp, *mean, *thr_eff;
  double* partial;
  int *cand_idx, *rowcount, *rowoff, *ncand;
  unsigned long long* topk_keys;
  int last_hp, last_wp;
};

extern "C" {

void dim_alike_destroy(dim_alike* h) {
  if (!h) return;
  dim_handle_release(&h->base);
  delete h;
}

int dim_alike_create(const dim_alike_weights* w, const dim_alike_config* cfg, int max_batch, int max_h, int max_w, int capacity, dim_alike** out) {
  DIM_REQUIRE(w && cfg && out, "dim_alike_create: null argument");
  const int c1 = cfg->c1, c2 = cfg->c2, c3 = cfg->c3, c4 = cfg->c4, dim = cfg->dim, q = cfg->dim / 4;
  const bool t = c1 == 8 && c2 == 16 && c3 == 32 && c4 == 64 && dim == 64 && cfg->single_head;
  const bool sm = c1 == 8 && c2 == 16 && c3 == 48 && c4 == 96 && dim == 96 && cfg->single_head;
  const bool n = c1 == 16 && c2 == 32 && c3 == 64 && c4 == 128 && dim == 128 && cfg->single_head;
  const bool l = c1 == 32 && c2 == 64 && c3 == 128 && c4 == 128 && dim == 128 && !cfg->single_head;
  DIM_REQUIRE(t || sm || n || l, "dim_alike_create: geometry (c1 %d, c2 %d, c3 %d, c4 %d, dim %d, single_head %d) is none of alike-t / s / n / l (AKM:15-56)", c1, c2,
              c3, c4, dim, cfg->single_head);
  DIM_REQUIRE(cfg->radius == 2, "dim_alike_create: radius %d (every ALIKE model uses 2, AKM:23-53)", cfg->radius);
  const int stride = cfg->desc_stride == 0 ? dim : cfg->desc_stride;
  DIM_REQUIRE(stride >= dim && stride % 4 == 0 && stride <= 128, "dim_alike_create: desc_stride %d must be 0 or a multiple of 4 in [dim = %d, 128]", cfg->desc_stride, dim);
  const int want = cfg->top_k > 0 ? cfg->top_k : cfg->n_limit;
  DIM_REQUIRE(capacity > 0 && capacity <= 32768, "dim_alike_create: capacity %d outside [1, 32768]", capacity);
  DIM_REQUIRE(want > 0 && want <= capacity, "dim_alike_create: capacity %d must cover %s %d", capacity, cfg->top_k > 0 ? "top_k" : "n_limit", want);
  DIM_REQUIRE(max_batch > 0 && max_batch <= 64, "dim_alike_create: max_batch %d outside [1, 64]", max_batch);
  DIM_REQUIRE(max_h >= 16 && max_w >= 16, "dim_alike_create: max_h %d / max_w %d below 16", max_h, max_w);
  DIM_REQUIRE(w->convhead2 && (l ? w->convhead1 != nullptr : w->convhead1 == nullptr), "dim_alike_create: convhead1 must be given for alike-l only");
  std::unique_ptr<dim_alike, void (*)(dim_alike*)> guard(new dim_alike(), dim_alike_destroy);
  dim_alike* const h = guard.get();
  DimHandleBase* const hb = &h->base;
  h->cfg = *cfg; h->stride = stride;
  h->max_batch = max_batch; h->max_h = max_h; h->max_w = max_w; h->capacity = capacity;

  // eval-mode BatchNorm as y = x * sc + bi (AKN:28-29,72-76): sc = weight / sqrt(running_var + 1e-5), bi = bias - running_mean * sc
  const int bnc[8] = {c1, c1, c2, c2, c3, c3, c4, c4};
  std::vector<double> sc[8], bi[8];
  for (int i = 0; i < 8; ++i) {
    DIM_REQUIRE(w->bn_weight[i] && w->bn_bias[i] && w->bn_mean[i] && w->bn_var[i], "dim_alike_create: BatchNorm layer %d has a null tensor", i);
    sc[i].resize(bnc[i]); bi[i].resize(bnc[i]);
    for (int c = 0; c < bnc[i]; ++c) {
      DIM_REQUIRE(w->bn_var[i][c] >= 0.0f, "dim_alike_create: BatchNorm layer %d has a negative running_var", i);
      sc[i][c] = (double)w->bn_weight[i][c] / sqrt((double)w->bn_var[i][c] + 1e-5);
      bi[i][c] = (double)w->bn_bias[i][c] - (double)w->bn_mean[i][c] * sc[i][c];
    }
  }
  // 3x3 layers: i even = the block's conv1 (ci -> co), i odd = its conv2 (co -> co) + downsample rows (blocks 2..4)
  const float* cw[8] = {w->block1_conv1, w->block1_conv2, w->block2_conv1, w->block2_conv2, w->block3_conv1, w->block3_conv2, w->block4_conv1, w->block4_conv2};
  const float* dsw[4] = {nullptr, w->block2_ds_w, w->block3_ds_w, w->block4_ds_w};
  const float* dsb[4] = {nullptr, w->block2_ds_b, w->block3_ds_b, w->block4_ds_b};
  const int cin_of[4] = {3, c1, c2, c3}, cout_of[4] = {c1, c2, c3, c4};
  for (int i = 0; i < 8; ++i) {
    const int blk = i / 2, co = cout_of[blk], ci = (i & 1) ? co : cin_of[blk];
    DIM_REQUIRE(cw[i], "dim_alike_create: 3x3 convolution %d is null", i);
    NhwcConvLayer& L = h->L[i];
    L.taps = 9; L.cin_pad = dim_pad16(ci);
    L.cin2_pad = ((i & 1) && blk > 0) ? dim_pad16(cin_of[blk]) : 0;
    const int K = 9 * L.cin_pad + L.cin2_pad;
    std::vector<float> kn((size_t)K * co, 0.0f), bias(co);
    nhwc_conv_pack_oihw(kn, co, 0, cw[i], co, ci, 3, L.cin_pad, &sc[i]);
    for (int c = 0; c < co; ++c) bias[c] = (float)bi[i][c];
    if (L.cin2_pad) {
      DIM_REQUIRE(dsw[blk] && dsb[blk], "dim_alike_create: block%d.downsample is null", blk + 1);
      nhwc_conv_pack_oihw(kn, co, 9 * L.cin_pad, dsw[blk], co, cin_of[blk], 1, L.cin2_pad, nullptr);
      for (int c = 0; c < co; ++c) bias[c] = (float)(bi[i][c] + (double)dsb[blk][c]);
    }
    DIM_TRY(nhwc_conv_upload(hb, &L, kn, K, co, bias));
  }
  {  // aggregation: conv2 / conv3 / conv4 (1x1, bias-free, ReLU; AKN:167-169) as layers; conv1 (AKN:166) is evaluated per pixel by the head kernels
    const float* aw[3] = {w->conv2, w->conv3, w->conv4};
    const int aci[3] = {c2, c3, c4};
    for (int g = 0; g < 3; ++g) {
      DIM_REQUIRE(aw[g], "dim_alike_create: conv%d is null", g + 2);
      NhwcConvLayer& L = h->A[g];
      L.taps = 1; L.cin_pad = dim_pad16(aci[g]); L.cin2_pad = 0;
      std::vector<float> kn((size_t)L.cin_pad * q, 0.0f), bias(q, 0.0f);
      nhwc_conv_pack_oihw(kn, q, 0, aw[g], q, aci[g], 1, L.cin_pad, nullptr);
      DIM_TRY(nhwc_conv_upload(hb, &L, kn, L.cin_pad, q, bias));
    }
    DIM_REQUIRE(w->conv1, "dim_alike_create: conv1 is null");
    std::vector<float> w1((size_t)dim_pad16(c1) * q, 0.0f);
    nhwc_conv_pack_oihw(w1, q, 0, w->conv1, q, c1, 1, dim_pad16(c1), nullptr);
    DIM_TRY(dim_upload_f32(hb, &h->w1, w1));
  }
  {  // heads (AKN:176-181): [K = dim][N = dim] operands; the score row of convhead2 on its own
    std::vector<float> kn((size_t)dim * dim);
    for (int o = 0; o < dim; ++o)
      for (int k = 0; k < dim; ++k) kn[(size_t)k * dim + o] = w->convhead2[(size_t)o * dim + k];
    DIM_TRY(dim_upload_f32(hb, &h->h2_w, kn));
    DIM_TRY(dim_upload_gemm_split(hb, &h->g_h2, kn.data(), dim, dim, 128, 2));
    DIM_TRY(dim_upload_f32(hb, &h->ws, w->convhead2 + (size_t)dim * dim, dim));
    h->h1_w = nullptr;
    if (l) {
      for (int o = 0; o < dim; ++o)
        for (int k = 0; k < dim; ++k) kn[(size_t)k * dim + o] = w->convhead1[(size_t)o * dim + k];
      DIM_TRY(dim_upload_f32(hb, &h->h1_w, kn));
      DIM_TRY(dim_upload_gemm_split(hb, &h->g_h1, kn.data(), dim, dim, 128, 2));
    }
  }
  const size_t B = max_batch, Hp = ((size_t)max_h + 31) / 32 * 32, Wp = ((size_t)max_w + 31) / 32 * 32, NP = Hp * Wp, cap = capacity;
  const size_t p1 = dim_pad16(c1), p2 = dim_pad16(c2), p3 = dim_pad16(c3), p4 = dim_pad16(c4), fq = dim_pad16(q);
  DIM_TRY(dim_dev_alloc(hb, &h->t1, B * NP * p1)); DIM_TRY(dim_dev_alloc(hb, &h->x1, B * NP * p1)); DIM_TRY(dim_dev_alloc(hb, &h->p2, B * NP / 4 * p1));
  DIM_TRY(dim_dev_alloc(hb, &h->t2, B * NP / 4 * p2)); DIM_TRY(dim_dev_alloc(hb, &h->x2, B * NP / 4 * p2)); DIM_TRY(dim_dev_alloc(hb, &h->p3, B * NP / 64 * p2));
  DIM_TRY(dim_dev_alloc(hb, &h->t3, B * NP / 64 * p3)); DIM_TRY(dim_dev_alloc(hb, &h->x3, B * NP / 64 * p3)); DIM_TRY(dim_dev_alloc(hb, &h->p4, B * NP / 1024 * p3));
  DIM_TRY(dim_dev_alloc(hb, &h->t4, B * NP / 1024 * p4)); DIM_TRY(dim_dev_alloc(hb, &h->x4, B * NP / 1024 * p4));
  DIM_TRY(dim_dev_alloc(hb, &h->f2, B * NP / 4 * fq)); DIM_TRY(dim_dev_alloc(hb, &h->f3, B * NP / 64 * fq)); DIM_TRY(dim_dev_alloc(hb, &h->f4, B * NP / 1024 * fq));
  DIM_TRY(dim_dev_alloc(hb, &h->q2, B * NP / 4)); DIM_TRY(dim_dev_alloc(hb, &h->q3, B * NP / 64)); DIM_TRY(dim_dev_alloc(hb, &h->q4, B * NP / 1024));
  DIM_TRY(dim_dev_alloc(hb, &h->score, B * NP)); DIM_TRY(dim_dev_alloc(hb, &h->nms, B * NP));
  h->rows_cap = 4 * cap;
  if (l && h->rows_cap < (size_t)AK_BAND_PIXELS + Wp) h->rows_cap = (size_t)AK_BAND_PIXELS + Wp;
  DIM_TRY(dim_dev_alloc(hb, &h->X, B * h->rows_cap * dim)); DIM_TRY(dim_dev_alloc(hb, &h->Y, B * h->rows_cap * dim));
  DIM_TRY(dim_dev_alloc(hb, &h->cand_score, B * NP)); DIM_TRY(dim_dev_alloc(hb, &h->cand_idx, B * NP)); DIM_TRY(dim_dev_alloc(hb, &h->rowcount, B * Hp));
  DIM_TRY(dim_dev_alloc(hb, &h->rowoff, B * Hp)); DIM_TRY(dim_dev_alloc(hb, &h->ncand, B)); DIM_TRY(dim_dev_alloc(hb, &h->kpts_px, B * cap * 2));
  DIM_TRY(dim_dev_alloc(hb, &h->sc_tmp, B * cap)); DIM_TRY(dim_dev_alloc(hb, &h->kpts_norm, B * cap * 2)); DIM_TRY(dim_dev_alloc(hb, &h->disp, B * cap));
  DIM_TRY(dim_dev_alloc(hb, &h->mean, B)); DIM_TRY(dim_dev_alloc(hb, &h->thr_eff, B)); DIM_TRY(dim_dev_alloc(hb, &h->partial, B * 256));
  h->topk_keys = nullptr;
  if (topk_scratch_keys(max_batch, capacity)) DIM_TRY(dim_dev_alloc(hb, &h->topk_keys, topk_scratch_keys(max_batch, capacity)));
  *out = guard.release();
  return 0;
}

int dim_alike_extract(dim_alike* h, const float* images_dev, int batch, int H, int W, float* kpts_xy_dev, float* scores_dev, float* desc_dev,
                      int32_t* n_kpts_dev, void* stream) {
  DIM_REQUIRE(h && images_dev && kpts_xy_dev && scores_dev && desc_dev && n_kpts_dev, "dim_alike_extract: null argument");
  DimTuneScope tune_scope(&h->base);
  DIM_REQUIRE(batch >= 1 && batch <= h->max_batch, "dim_alike_extract: batch %d outside [1,%d]", batch, h->max_batch);
  DIM_REQUIRE(H >= 16 && W >= 16 && H <= h->max_h && W <= h->max_w, "dim_alike_extract: image %dx%d outside the handle's %dx%d", H, W, h->max_h, h->max_w);
  hipStream_t s = (hipStream_t)stream;
  const int c1 = h->cfg.c1, dim = h->cfg.dim, q = dim / 4, cap = h->capacity;
  const int Hp = (H + 31) / 32 * 32, Wp = (W + 31) / 32 * 32;   // zeros at the bottom and right only (AKM:105-113)
  const int H2 = Hp / 2, W2 = Wp / 2, H8 = Hp / 8, W8 = Wp / 8, H32 = Hp / 32, W32 = Wp / 32;
  const bool x3 = dim_precision_mode() == 2;   // fp16x3 on the matrix cores; every other mode runs the fp32 MFMA forms
  unsigned* const sat = dim_sat_counter(DIM_SAT_ALIKE);
  auto conv = [&](const NhwcConvLayer& L, const float* in, const float* in2, float* out, float* pooled, int pool, int Hh, int Ww, bool img) -> int {
    NhwcConv a;
    a.in = in; a.cin_pad = L.cin_pad; a.taps = L.taps; a.in2 = in2; a.cin2_pad = in2 ? L.cin2_pad : 0;
    a.img3 = img ? 1 : 0; a.in_h = img ? H : Hh; a.in_w = img ? W : Ww;   // the image layer reads the unpadded image into the padded frame
    a.wx = &L.wx; a.w32 = L.w32; a.bias = L.bias; a.n_pad = L.n_pad; a.out = out; a.out_c = L.out_c; a.pooled = pooled; a.pool = pool;
    a.relu = 1; a.batch = batch; a.H = Hh; a.W = Ww; a.sat = sat;
    return launch_nhwc_conv(a, x3, s);
  };
  // encoder (AKN:157-163): block1 on the padded frame, max-pools fused into the epilogues that feed them
  DIM_RUN(conv(h->L[0], images_dev, nullptr, h->t1, nullptr, 0, Hp, Wp, true));
  DIM_RUN(conv(h->L[1], h->t1, nullptr, h->x1, h->p2, 2, Hp, Wp, false));
  DIM_RUN(conv(h->L[2], h->p2, nullptr, h->t2, nullptr, 0, H2, W2, false));
  DIM_RUN(conv(h->L[3], h->t2, h->p2, h->x2, h->p3, 4, H2, W2, false));
  DIM_RUN(conv(h->L[4], h->p3, nullptr, h->t3, nullptr, 0, H8, W8, false));
  DIM_RUN(conv(h->L[5], h->t3, h->p3, h->x3, h->p4, 4, H8, W8, false));
  DIM_RUN(conv(h->L[6], h->p4, nullptr, h->t4, nullptr, 0, H32, W32, false));
  DIM_RUN(conv(h->L[7], h->t4, h->p4, h->x4, nullptr, 0, H32, W32, false));
  // aggregation at the levels' own resolutions (AKN:167-169)
  DIM_RUN(conv(h->A[0], h->x2, nullptr, h->f2, nullptr, 0, H2, W2, false));
  DIM_RUN(conv(h->A[1], h->x3, nullptr, h->f3, nullptr, 0, H8, W8, false));
  DIM_RUN(conv(h->A[2], h->x4, nullptr, h->f4, nullptr, 0, H32, W32, false));
  const int fq = h->A[0].out_c;
  const AkFeat F{h->x1, h->f2, h->f3, h->f4, h->w1, Hp, Wp, dim_pad16(c1), q, fq};
  auto head_gemm = [&](const float* Ain, const float* w32, const SplitWeights& wx, float* Cout, int M, const int* rows, int relu) -> int {
    GemmArgs g;
    g.A0 = Ain; g.lda0 = dim; g.strideA0 = (long long)h->rows_cap * dim; g.B = w32; g.ldb = dim;
    g.C = Cout; g.ldc = dim; g.strideC = (long long)h->rows_cap * dim; g.M = M; g.N = dim; g.K = dim;
    g.rows = rows; g.rows_scale = rows ? 4 : 1; g.relu = relu;
    if (x3) { g.set_split(wx); g.sat = sat; return launch_gemm_x6(g, batch, s); }
    return launch_gemm(g, batch, s);
  };
  if (h->cfg.single_head) {
    // score = sigmoid(w_s . x1234) with the three up-sampled groups projected to ONE channel before the interpolation (exact in real
    // arithmetic: the interpolation is linear and convhead2 follows it without an activation, AKN:170-181)
    DIM_RUN(launch_ak_project(h->f2, fq, q, h->ws + q, h->q2, batch * H2 * W2, s));
    DIM_RUN(launch_ak_project(h->f3, fq, q, h->ws + 2 * q, h->q3, batch * H8 * W8, s));
    DIM_RUN(launch_ak_project(h->f4, fq, q, h->ws + 3 * q, h->q4, batch * H32 * W32, s));
    DIM_RUN(launch_ak_score(F, h->ws, h->q2, h->q3, h->q4, h->score, batch, H, W, s));
  } else {
    // alike-l: relu(convhead1 . x1234) is dense work (AKN:176-177): x1234 is assembled per row band, the 128 x 128 product runs on the
    // matrix cores and the band is contracted with w_s; the band scratch does not depend on the image height
    const int band = AK_BAND_PIXELS / W > 0 ? AK_BAND_PIXELS / W : 1;
    for (int y0 = 0; y0 < H; y0 += band) {
      const int rows = (y0 + band <= H ? band : H - y0) * W;
      DIM_RUN(launch_ak_rows(F, nullptr, nullptr, 0, y0, rows, h->X, dim, (long long)h->rows_cap * dim, batch, H, W, sat, s));
      DIM_RUN(head_gemm(h->X, h->h1_w, h->g_h1, h->Y, rows, nullptr, 1));
      DIM_RUN(launch_ak_contract(h->Y, dim, (long long)h->rows_cap * dim, h->ws, dim, h->score, y0, rows, batch, H, W, s));
    }
  }
  // DKD (AKD:98-134): NMS radius 2 (hard-coded, AKD:102), asymmetric border, top-k or threshold selection
  DIM_RUN(launch_nms(h->score, h->nms, batch, H, W, 2, s));
  DIM_RUN(launch_ak_border(h->nms, batch, H, W, s));
  if (h->cfg.top_k > 0) {
    // torch.topk over the border-cleared NMS map (AKD:111-113): every positive maximum is a candidate, sorted; zero-valued pixels fill up
    DIM_RUN(launch_select_ex(h->nms, batch, H, W, 0.f, nullptr, 0, h->rowcount, h->rowoff, h->ncand, h->cand_score, h->cand_idx, 0, s));
    DIM_RUN(launch_topk(h->cand_score, h->cand_idx, h->ncand, batch, H, W, h->cfg.top_k, cap, h->kpts_px, h->sc_tmp, n_kpts_dev, h->topk_keys, 1, s));
    DIM_RUN(launch_topk_zero_fill(h->nms, batch, H, W, 0.f, 0, h->cfg.top_k, cap, h->kpts_px, h->sc_tmp, n_kpts_dev, s));
  } else {
    DIM_RUN(launch_al_mean(h->score, batch, H * W, h->partial, h->mean, s));
    const float thr = (float)h->cfg.scores_th;
    if (thr > 0.f) DIM_RUN(launch_select_ex(h->nms, batch, H, W, thr, nullptr, 0, h->rowcount, h->rowoff, h->ncand, h->cand_score, h->cand_idx, 1, s));
    DIM_RUN(launch_al_pick_threshold(h->ncand, h->mean, thr, h->thr_eff, batch, s));   // the mean when scores_th <= 0 or nothing passes (AKD:115-122), per image
    DIM_RUN(launch_select_ex(h->nms, batch, H, W, 0.f, h->thr_eff, 0, h->rowcount, h->rowoff, h->ncand, h->cand_score, h->cand_idx, 0, s));
    DIM_RUN(launch_topk(h->cand_score, h->cand_idx, h->ncand, batch, H, W, h->cfg.n_limit, cap, h->kpts_px, h->sc_tmp, n_kpts_dev, h->topk_keys, 0, s));
  }
  // soft-argmax refinement over the 5x5 window, temperature 0.1 (AKD:139-178); its bilinear score sample is ALIKE's `scores` (AKD:180-187)
  DIM_RUN(launch_al_dkd_refine(h->score, h->kpts_px, n_kpts_dev, h->kpts_norm, h->disp, scores_dev, kpts_xy_dev, batch, H, W, cap, 2, s));
  // sparse descriptor head: x1234 at the four pixels around every keypoint, convhead (1 +) 2 on those rows only
  DIM_RUN(launch_ak_rows(F, h->kpts_norm, n_kpts_dev, cap, 0, 0, h->X, dim, (long long)h->rows_cap * dim, batch, H, W, sat, s));
  const float* D = h->Y;
  if (h->cfg.single_head) {
    DIM_RUN(head_gemm(h->X, h->h2_w, h->g_h2, h->Y, 4 * cap, n_kpts_dev, 0));
  } else {
    DIM_RUN(head_gemm(h->X, h->h1_w, h->g_h1, h->Y, 4 * cap, n_kpts_dev, 1));
    DIM_RUN(head_gemm(h->Y, h->h2_w, h->g_h2, h->X, 4 * cap, n_kpts_dev, 0));
    D = h->X;
  }
  DIM_RUN(launch_ak_desc_blend(D, dim, (long long)h->rows_cap * dim, h->kpts_norm, n_kpts_dev, desc_dev, dim, h->stride, cap, batch, H, W, s));
  h->last_hp = Hp; h->last_wp = Wp;
  return 0;
}

int dim_alike_debug_buffers(dim_alike* h, const float** score_map, const float** nms_map, int* hp, int* wp) {
  DIM_REQUIRE(h, "dim_alike_debug_buffers: null handle");
  if (score_map) *score_map = h->score;
  if (nms_map) *nms_map = h->nms;
  if (hp) *hp = h->last_hp;
  if (wp) *wp = h->last_wp;
  return 0;
}

}  // extern "C"
