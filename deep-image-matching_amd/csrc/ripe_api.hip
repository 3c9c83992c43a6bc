// dim_ripe_* : resident RIPE extractor (C ABI in include/dim_hip.h) and the operator entries of its own kernels.
// Replaces RIPE.detectAndCompute (thirdparty/RIPE/ripe/models/ripe.py:201-260 = RPM) over VGG (models/backbones/vgg.py = RPV, vgg_utils.py = RPU,
// backbone_base.py = RPB) and HyperColumnFeatures (models/upsampler/hypercolumn_features.py = RPH) as RIPEExtractor (extractors/ripe.py) drives it.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/dim_hip.h"
#include "netvlad_kernels.h"
#include "ripe_kernels.h"
#include "sp_kernels.h"

namespace {
constexpr int RP_NL = 12;
// torchvision's vgg19_bn up to the fourth pool: cin, cout, 1 = the map is kept and pooled behind this layer (RPU:117-124)
struct RpGeo { int ci, co, keep; };
const RpGeo RP_VGG[RP_NL] = {{3, 64, 0}, {64, 64, 1}, {64, 128, 0}, {128, 128, 1}, {128, 256, 0}, {256, 256, 0}, {256, 256, 0}, {256, 256, 1},
                             {256, 512, 0}, {512, 512, 0}, {512, 512, 0}, {512, 512, 1}};
// ConvRefiner per scale 8, 4, 2, 1 (RPV:38-71): channels of the encoder map, of the context, hidden, out
struct RpDec { int cf, cc, hid, out; };
const RpDec RP_DEC[4] = {{512, 0, 512, 257}, {256, 256, 256, 129}, {128, 128, 128, 65}, {64, 64, 64, 2}};

// a 1 x 1 convolution as a GEMM over the [pixels][K] rows: both splits of the [K][N] operand, bias [N]
struct RpLin { SplitWeights w[3]; float* bias = nullptr; int K = 0, N = 0; };
struct RpDw { float *w = nullptr, *bias = nullptr; };

// eval-mode BatchNorm behind a convolution, folded in fp64: y = sc (conv + b - mean) + beta, sc = gamma / sqrt(var + 1e-5)
int rp_fold(const dim_ripe_convbn& c, int co, size_t w_per_co, const char* what, std::vector<double>* sc, std::vector<float>* bias) {
  DIM_REQUIRE(c.w && c.b && c.gamma && c.beta && c.mean && c.var, "dim_ripe_create: %s has a null tensor", what);
  DIM_REQUIRE(dim_all_finite(c.w, (size_t)co * w_per_co) && dim_all_finite(c.b, co) && dim_all_finite(c.gamma, co) && dim_all_finite(c.beta, co) &&
                  dim_all_finite(c.mean, co) && dim_all_finite(c.var, co),
              "dim_ripe_create: %s holds a non-finite value", what);
  sc->resize(co); bias->resize(co);
  for (int i = 0; i < co; ++i) {
    DIM_REQUIRE(c.var[i] >= 0.0f, "dim_ripe_create: %s has a negative running_var", what);
    (*sc)[i] = (double)c.gamma[i] / sqrt((double)c.var[i] + 1e-5);
    (*bias)[i] = (float)(((double)c.b[i] - (double)c.mean[i]) * (*sc)[i] + (double)c.beta[i]);
  }
  return 0;
}

// (co, ci, 1, 1) weight, optionally scaled per output channel -> RpLin
int rp_upload_lin(DimHandleBase* hb, RpLin* L, const float* w, const float* b, int co, int ci, const std::vector<double>* sc, const std::vector<float>* bias,
                  const char* what) {
  DIM_REQUIRE(w && (b || bias), "dim_ripe_create: %s has a null tensor", what);
  DIM_REQUIRE(dim_all_finite(w, (size_t)co * ci) && (bias || dim_all_finite(b, co)), "dim_ripe_create: %s holds a non-finite value", what);
  std::vector<float> kn((size_t)ci * co);
  for (int o = 0; o < co; ++o)
    for (int i = 0; i < ci; ++i) kn[(size_t)i * co + o] = sc ? (float)((double)w[(size_t)o * ci + i] * (*sc)[o]) : w[(size_t)o * ci + i];
  L->K = ci; L->N = co;
  const int n_pad = (co + 127) / 128 * 128;
  for (int mode = 1; mode <= 2; ++mode) DIM_TRY(dim_upload_gemm_split(hb, &L->w[mode], kn.data(), ci, co, n_pad, mode));
  if (bias) DIM_TRY(dim_upload_f32(hb, &L->bias, *bias));
  else DIM_TRY(dim_upload_f32(hb, &L->bias, b, co));
  return 0;
}
}  // namespace

struct dim_ripe {
  DimHandleBase base;   // first member: dim_handle_tune_set
  int max_batch, max_h, max_w, capacity;
  float *w1, *enc_bias[RP_NL];
  SplitWeights wsp[3][RP_NL];   // [mode 1 | 2][layer 1 ..]
  RpLin b1_0[4], b1_3[4], pw[4][8], outc[4], desc;
  RpDw dw[4][8];
  double *stat_partial, *stats;
  float *f[4], *buf[4], *dout, *logit[2], *heat, *key, *max_partial, *mapmax;
  float *cand_score, *kpts_px, *raw_scores, *rows, *lin;
  int *cand_idx, *rowcount, *rowoff, *ncand;
  unsigned long long* topk_keys;
  int last_batch, last_h, last_w;
};

extern "C" {

void dim_ripe_destroy(dim_ripe* h) {
  if (!h) return;
  dim_handle_release(&h->base);
  delete h;
}

int dim_ripe_create(const dim_ripe_weights* w, int max_batch, int max_h, int max_w, int capacity, dim_ripe** out) {
  DIM_REQUIRE(w && out, "dim_ripe_create: null argument");
  DIM_REQUIRE(max_batch > 0 && max_batch <= 64, "dim_ripe_create: max_batch %d outside [1, 64]", max_batch);
  DIM_REQUIRE(max_h >= 16 && max_w >= 16, "dim_ripe_create: max_h %d / max_w %d below 16 (three pools ahead of the coarsest map)", max_h, max_w);
  // the 64-channel fp32 map of one image at full resolution must fit one buffer descriptor (launch_conv3x3_x6_wide, launch_gemm_x6)
  DIM_REQUIRE((long long)max_h * max_w * 64 * 4 < 0x7FFFFFF0LL, "dim_ripe_create: %d x %d: the 64-channel map of one image exceeds 2 GiB (stay below 2^23 pixels)", max_h, max_w);
  DIM_REQUIRE(capacity > 0 && capacity <= 32768, "dim_ripe_create: capacity %d outside [1, 32768]", capacity);
  std::unique_ptr<dim_ripe, void (*)(dim_ripe*)> guard(new dim_ripe(), dim_ripe_destroy);
  dim_ripe* const h = guard.get();
  DimHandleBase* const hb = &h->base;
  h->max_batch = max_batch; h->max_h = max_h; h->max_w = max_w; h->capacity = capacity;
  h->last_batch = h->last_h = h->last_w = 0;

  char what[64];
  std::vector<double> sc;
  std::vector<float> bias;
  for (int l = 0; l < RP_NL; ++l) {
    const RpGeo& g = RP_VGG[l];
    snprintf(what, sizeof(what), "encoder convolution %d", l);
    DIM_RUN(rp_fold(w->enc[l], g.co, (size_t)g.ci * 9, what, &sc, &bias));
    DIM_TRY(dim_upload_f32(hb, &h->enc_bias[l], bias));
    std::vector<float> wf((size_t)g.co * g.ci * 9);
    for (int co = 0; co < g.co; ++co)
      for (size_t j = 0; j < (size_t)g.ci * 9; ++j) wf[(size_t)co * g.ci * 9 + j] = (float)((double)w->enc[l].w[(size_t)co * g.ci * 9 + j] * sc[co]);
    if (l == 0) {   // [(ci, dy, dx)][64]
      std::vector<float> k(27 * 64);
      for (int co = 0; co < 64; ++co)
        for (int j = 0; j < 27; ++j) k[(size_t)j * 64 + co] = wf[(size_t)co * 27 + j];
      DIM_TRY(dim_upload_f32(hb, &h->w1, k));
      continue;
    }
    for (int mode = 1; mode <= 2; ++mode) {
      std::vector<unsigned short> hx(conv_split_weight_elems(g.ci, g.co, mode));
      SplitWeights& sw = h->wsp[mode][l];
      prepare_conv_weights_split(wf.data(), g.ci, g.co, mode, hx.data(), &sw);
      DIM_TRY(dim_upload_split(hb, &sw, hx, mode, sw.n_pad));
    }
  }
  for (int d = 0; d < 4; ++d) {
    const RpDec& g = RP_DEC[d];
    const dim_ripe_refiner& r = w->dec[d];
    snprintf(what, sizeof(what), "decoder %d block1.0", d);
    DIM_RUN(rp_fold(r.block1_0, g.hid, g.cf + g.cc, what, &sc, &bias));
    DIM_RUN(rp_upload_lin(hb, &h->b1_0[d], r.block1_0.w, nullptr, g.hid, g.cf + g.cc, &sc, &bias, what));
    snprintf(what, sizeof(what), "decoder %d block1.3", d);
    DIM_RUN(rp_upload_lin(hb, &h->b1_3[d], r.block1_3_w, r.block1_3_b, g.hid, g.hid, nullptr, nullptr, what));
    for (int j = 0; j < 8; ++j) {
      snprintf(what, sizeof(what), "decoder %d hidden block %d", d, j);
      DIM_RUN(rp_fold(r.dw[j], g.hid, 25, what, &sc, &bias));
      std::vector<float> k((size_t)25 * g.hid);   // [tap][channel]
      for (int c = 0; c < g.hid; ++c)
        for (int t = 0; t < 25; ++t) k[(size_t)t * g.hid + c] = (float)((double)r.dw[j].w[(size_t)c * 25 + t] * sc[c]);
      DIM_TRY(dim_upload_f32(hb, &h->dw[d][j].w, k));
      DIM_TRY(dim_upload_f32(hb, &h->dw[d][j].bias, bias));
      DIM_RUN(rp_upload_lin(hb, &h->pw[d][j], r.pw_w[j], r.pw_b[j], g.hid, g.hid, nullptr, nullptr, what));
    }
    snprintf(what, sizeof(what), "decoder %d out_conv", d);
    DIM_RUN(rp_upload_lin(hb, &h->outc[d], r.out_w, r.out_b, g.out, g.hid, nullptr, nullptr, what));
  }
  DIM_RUN(rp_upload_lin(hb, &h->desc, w->desc_w, w->desc_b, RIPE_DESC_DIM, RIPE_HYPER_DIM, nullptr, nullptr, "conv_dim_reduction_coarse_desc"));

  const size_t B = max_batch, P = (size_t)max_h * max_w, cap = capacity;
  size_t hl = max_h, wl = max_w, dout = 0;
  for (int l = 0; l < 4; ++l) {
    DIM_TRY(dim_dev_alloc(hb, &h->f[l], B * hl * wl * (64u << l)));
    const size_t o = hl * wl * RP_DEC[3 - l].out;
    dout = o > dout ? o : dout;
    hl /= 2; wl /= 2;
  }
  for (int i = 0; i < 4; ++i) DIM_TRY(dim_dev_alloc(hb, &h->buf[i], B * P * 64));   // the largest map of either half: 64 channels at full resolution
  DIM_TRY(dim_dev_alloc(hb, &h->dout, B * dout));
  DIM_TRY(dim_dev_alloc(hb, &h->logit[0], B * P)); DIM_TRY(dim_dev_alloc(hb, &h->logit[1], B * P));
  DIM_TRY(dim_dev_alloc(hb, &h->heat, B * P)); DIM_TRY(dim_dev_alloc(hb, &h->key, B * P));
  DIM_TRY(dim_dev_alloc(hb, &h->stat_partial, B * ripe_stats_blocks(max_h, max_w) * 6)); DIM_TRY(dim_dev_alloc(hb, &h->stats, B * 6));
  DIM_TRY(dim_dev_alloc(hb, &h->max_partial, B * ripe_max_blocks((int)P))); DIM_TRY(dim_dev_alloc(hb, &h->mapmax, B));
  DIM_TRY(dim_dev_alloc(hb, &h->cand_score, B * P)); DIM_TRY(dim_dev_alloc(hb, &h->cand_idx, B * P));
  DIM_TRY(dim_dev_alloc(hb, &h->rowcount, B * max_h)); DIM_TRY(dim_dev_alloc(hb, &h->rowoff, B * max_h)); DIM_TRY(dim_dev_alloc(hb, &h->ncand, B));
  DIM_TRY(dim_dev_alloc(hb, &h->kpts_px, B * cap * 2)); DIM_TRY(dim_dev_alloc(hb, &h->raw_scores, B * cap));
  DIM_TRY(dim_dev_alloc(hb, &h->rows, B * cap * RIPE_HYPER_DIM)); DIM_TRY(dim_dev_alloc(hb, &h->lin, B * cap * RIPE_DESC_DIM));
  h->topk_keys = nullptr;
  if (topk_scratch_keys(max_batch, capacity)) DIM_TRY(dim_dev_alloc(hb, &h->topk_keys, topk_scratch_keys(max_batch, capacity)));
  *out = guard.release();
  return 0;
}

int dim_ripe_extract(dim_ripe* h, const float* images_dev, int batch, int H, int W, int top_k, float threshold, float* kpts_xy_dev, float* scores_dev,
                     float* desc_dev, int32_t* counts_dev, void* stream) {
  DIM_REQUIRE(h && images_dev && kpts_xy_dev && scores_dev && desc_dev && counts_dev, "dim_ripe_extract: null argument");
  DimTuneScope tune_scope(&h->base);
  DIM_REQUIRE(batch >= 1 && batch <= h->max_batch, "dim_ripe_extract: batch %d outside [1,%d]", batch, h->max_batch);
  DIM_REQUIRE(H >= 16 && W >= 16 && H <= h->max_h && W <= h->max_w, "dim_ripe_extract: image %dx%d outside [16x16, the handle's %dx%d]", H, W, h->max_h, h->max_w);
  DIM_REQUIRE(top_k > 0 && top_k <= h->capacity, "dim_ripe_extract: top_k %d outside [1, the handle's capacity %d]", top_k, h->capacity);
  DIM_REQUIRE(threshold >= 0.0f, "dim_ripe_extract: threshold %g below 0", (double)threshold);
  hipStream_t s = (hipStream_t)stream;
  const int mode = dim_precision_mode() == 2 ? 2 : 1;   // fp16x3 under the range guard, else the bf16x6 split (no range limit)
  unsigned* const sat = mode == 2 ? dim_sat_counter(DIM_SAT_RIPE) : nullptr;
  int hs[4], ws[4];
  for (int l = 0; l < 4; ++l) { hs[l] = H >> l; ws[l] = W >> l; }

  // ---- encoder (RPB:62-63, RPU:126-134): the map in front of every pool is kept; the fourth pool's output is never used ----
  dim_prof_begin(DIM_PROF_RIPE_ENCODER, s);
  DIM_RUN(launch_ripe_stats(images_dev, h->stat_partial, h->stats, batch, H, W, s));
  DIM_RUN(launch_ripe_conv1(images_dev, h->stats, h->w1, h->enc_bias[0], h->buf[0], batch, H, W, sat, s));
  {
    const float* cur = h->buf[0];
    int level = 0;
    for (int l = 1; l < RP_NL; ++l) {
      const RpGeo& g = RP_VGG[l];
      float* dst = g.keep ? h->f[level] : (cur == h->buf[0] ? h->buf[1] : h->buf[0]);
      DIM_RUN(launch_conv3x3_x6_wide(cur, h->wsp[mode][l], h->enc_bias[l], dst, batch, hs[level], ws[level], g.ci, g.co, 1, s, sat));
      cur = dst;
      if (g.keep && level < 3) {
        DIM_RUN(launch_nv_maxpool(cur, h->buf[0], batch, hs[level], ws[level], g.co, s));
        cur = h->buf[0];
        ++level;
      }
    }
  }
  dim_prof_end(DIM_PROF_RIPE_ENCODER, s);

  // ---- decoder (RPV:84-97), coarse to fine.  buf[0] = x0, buf[1] = block1's hidden / the depthwise output, buf[2] | buf[3] = the running x;
  // buf[2] also carries the resized context into the next scale's block1 ----
  auto lin = [&](const RpLin& L, const float* A0, int lda0, const float* A1, int lda1, float* C, int M, int relu, const float* R, int item_rows = 0,
                 const int* rows = nullptr) -> int {
    GemmArgs g;
    const long long stride_rows = item_rows ? item_rows : M;
    g.A0 = A0; g.lda0 = lda0; g.strideA0 = stride_rows * lda0;
    g.A1 = A1; g.lda1 = lda1; g.strideA1 = stride_rows * lda1; g.ksplit = A1 ? lda0 : 0;
    g.set_split(L.w[mode]);
    g.bias = L.bias;
    g.R = R; g.ldr = L.N; g.strideR = stride_rows * L.N;
    g.C = C; g.ldc = L.N; g.strideC = stride_rows * L.N;
    g.M = M; g.N = L.N; g.K = L.K; g.relu = relu; g.sat = sat; g.rows = rows;
    return launch_gemm_x6(g, batch, s);
  };
  const float* acc = nullptr;   // the running logit map, resized to the current scale
  for (int d = 0; d < 4; ++d) {
    const RpDec& g = RP_DEC[d];
    const int l = 3 - d, M = hs[l] * ws[l];
    dim_prof_begin(DIM_PROF_RIPE_DEC8 + d, s);
    DIM_RUN(lin(h->b1_0[d], h->f[l], g.cf, g.cc ? h->buf[2] : nullptr, g.cc, h->buf[1], M, 1, nullptr));
    DIM_RUN(lin(h->b1_3[d], h->buf[1], g.hid, nullptr, 0, h->buf[0], M, 0, nullptr));
    const float* cur = h->buf[0];
    for (int j = 0; j < 8; ++j) {
      float* nxt = (j & 1) ? h->buf[3] : h->buf[2];
      DIM_RUN(launch_ripe_dw5x5(cur, h->dw[d][j].w, h->dw[d][j].bias, h->buf[1], batch, hs[l], ws[l], g.hid, sat, s));
      DIM_RUN(lin(h->pw[d][j], h->buf[1], g.hid, nullptr, 0, nxt, M, 0, j == 7 ? h->buf[0] : nullptr));   // the last block adds x0 (RPU:99-100)
      cur = nxt;
    }
    DIM_RUN(launch_ripe_div14(h->buf[3], (size_t)batch * M * g.hid, s));
    DIM_RUN(lin(h->outc[d], h->buf[3], g.hid, nullptr, 0, h->dout, M, 0, nullptr));   // [pixels][out]: channel 0 = the logit, 1 .. = the context
    float* sum = d == 3 ? h->heat : h->logit[0];
    DIM_RUN(launch_ripe_logit_add(acc, h->dout, g.out, sum, batch, M, s));
    if (d < 3) {
      DIM_RUN(launch_ripe_resize_bilinear(sum, 1, 0, 1, batch, hs[l], ws[l], h->logit[1], hs[l - 1], ws[l - 1], s));
      DIM_RUN(launch_ripe_resize_bilinear(h->dout, g.out, 1, g.out - 1, batch, hs[l], ws[l], h->buf[2], hs[l - 1], ws[l - 1], s));
      acc = h->logit[1];
    }
    dim_prof_end(DIM_PROF_RIPE_DEC8 + d, s);
  }

  // ---- detection (RPM:201-222, 262-267): the heat map is the logit map (the non-linearity is the identity) ----
  dim_prof_begin(DIM_PROF_RIPE_DETECT, s);
  DIM_RUN(launch_ripe_nms3(h->heat, h->key, threshold, batch, H, W, s));
  DIM_RUN(launch_ripe_map_max(h->heat, h->max_partial, h->mapmax, batch, H * W, s));
  DIM_RUN(launch_select_ex(h->key, batch, H, W, 0.f, nullptr, 0, h->rowcount, h->rowoff, h->ncand, h->cand_score, h->cand_idx, 0, s));
  DIM_REQUIRE(top_k <= 4096 || h->topk_keys != nullptr, "dim_ripe_extract: top_k %d needs the handle's key table", top_k);
  DIM_RUN(launch_topk(h->cand_score, h->cand_idx, h->ncand, batch, H, W, top_k, h->capacity, kpts_xy_dev, h->raw_scores, (int*)counts_dev, h->topk_keys, 1, s));
  dim_prof_end(DIM_PROF_RIPE_DETECT, s);

  // ---- descriptors of the selected keypoints (RPM:269-283, RPH) ----
  RipeLevels lv;
  for (int l = 0; l < 4; ++l) { lv.f[l] = h->f[l]; lv.h[l] = hs[l]; lv.w[l] = ws[l]; }
  dim_prof_begin(DIM_PROF_RIPE_DESC, s);
  DIM_RUN(launch_ripe_hypercolumn(lv, kpts_xy_dev, (const int*)counts_dev, h->rows, h->capacity, batch, H, W, s));
  DIM_RUN(lin(h->desc, h->rows, RIPE_HYPER_DIM, nullptr, 0, h->lin, h->capacity, 0, nullptr, h->capacity, (const int*)counts_dev));
  DIM_RUN(launch_ripe_desc_finish(h->lin, h->raw_scores, h->mapmax, (const int*)counts_dev, desc_dev, scores_dev, h->capacity, batch, s));
  dim_prof_end(DIM_PROF_RIPE_DESC, s);
  h->last_batch = batch; h->last_h = H; h->last_w = W;
  return 0;
}

int dim_ripe_debug_buffers(dim_ripe* h, const float** heat, const float** maps4, int* hs4, int* ws4, int* batch) {
  DIM_REQUIRE(h, "dim_ripe_debug_buffers: null handle");
  if (heat) *heat = h->heat;
  for (int l = 0; l < 4; ++l) {
    if (maps4) maps4[l] = h->f[l];
    if (hs4) hs4[l] = h->last_h >> l;
    if (ws4) ws4[l] = h->last_w >> l;
  }
  if (batch) *batch = h->last_batch;
  return 0;
}

int dim_op_ripe_dw5x5_f32(const float* in_dev, const float* w_dev, const float* bias_dev, float* out_dev, int batch, int H, int W, int C, void* stream) {
  DIM_REQUIRE(in_dev && w_dev && bias_dev && out_dev, "dim_op_ripe_dw5x5_f32: null argument");
  DIM_REQUIRE(batch >= 1 && H >= 1 && W >= 1 && (long long)batch * H * W * C <= 0x7fffffffLL, "dim_op_ripe_dw5x5_f32: bad size %d x %d x %d x %d", batch, H, W, C);
  return launch_ripe_dw5x5(in_dev, w_dev, bias_dev, out_dev, batch, H, W, C, dim_precision_mode() == 2 ? dim_sat_counter(DIM_SAT_OP) : nullptr, (hipStream_t)stream);
}

int dim_op_ripe_resize_bilinear_f32(const float* in_dev, int ld, int c_off, int C, int batch, int h, int w, float* out_dev, int H, int W, void* stream) {
  DIM_REQUIRE(in_dev && out_dev && batch >= 1, "dim_op_ripe_resize_bilinear_f32: null argument or batch %d", batch);
  return launch_ripe_resize_bilinear(in_dev, ld, c_off, C, batch, h, w, out_dev, H, W, (hipStream_t)stream);
}

int dim_op_ripe_nms3_f32(const float* heat_dev, float* key_dev, float threshold, int batch, int H, int W, void* stream) {
  DIM_REQUIRE(heat_dev && key_dev && batch >= 1 && H >= 1 && W >= 1, "dim_op_ripe_nms3_f32: null argument or bad size %d x %d x %d", batch, H, W);
  return launch_ripe_nms3(heat_dev, key_dev, threshold, batch, H, W, (hipStream_t)stream);
}

int dim_op_ripe_hypercolumn_f32(const float* const* maps4, const int* hs4, const int* ws4, const float* kpts_dev, const int32_t* n_kpts_dev, float* rows_dev,
                                int capacity, int batch, int H, int W, void* stream) {
  DIM_REQUIRE(maps4 && hs4 && ws4 && kpts_dev && n_kpts_dev && rows_dev, "dim_op_ripe_hypercolumn_f32: null argument");
  RipeLevels lv;
  for (int l = 0; l < 4; ++l) {
    DIM_REQUIRE(maps4[l] && hs4[l] >= 1 && ws4[l] >= 1, "dim_op_ripe_hypercolumn_f32: level %d is null or empty", l);
    lv.f[l] = maps4[l]; lv.h[l] = hs4[l]; lv.w[l] = ws4[l];
  }
  return launch_ripe_hypercolumn(lv, kpts_dev, (const int*)n_kpts_dev, rows_dev, capacity, batch, H, W, (hipStream_t)stream);
}

}  // extern "C"
