// dim_sp_* : resident SuperPoint extractor (C ABI in include/dim_hip.h).
// Replaces SuperPoint.__init__/forward (SPN:101-227) as driven by
// SuperPointExtractor._extract (extractors/superpoint.py:107-132).
//
// HBM layout: every activation is NHWC fp32 ([batch][H][W][C]); 1x1 convolutions
// are therefore plain GEMMs over pixels; the descriptor head's output stays
// un-normalised in HBM and is normalised only at the <= 4 cells each keypoint
// touches (sample_desc_kernel), which is algebraically the reference's
// normalise-then-sample (SPN:215,218-221).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/dim_hip.h"
#include "sp_kernels.h"

struct dim_sp {
  DimHandleBase base;   // first member: dim_handle_tune_set
  dim_sp_config cfg;
  int max_batch, max_h, max_w, capacity;
  // weights (device)
  float* w1a; float* wk[12]; float* bias[12];
  SplitWeights wsw[12];     // Winograd F(2,3)-transformed fp16x3 weights (conv_wg.hip) of the layers that have the variant (conv1b)
  SplitWeights wsp[3][12];  // [precision mode 1 = bf16x6, 2 = fp16x3] pre-split 3x3 weights (conv_x6.hip); empty for conv1a and the 1x1 layers
  // activations
  float *a1, *b1, *a2, *b2, *a3, *b3, *a4, *x, *pa, *logits, *da, *dd, *smap, *nms, *cand_score;
  int *cand_idx, *rowcount, *rowoff, *ncand;
  unsigned long long* topk_keys;   // launch_topk's global key table (max_keypoints > 4096 only)
  int last_h, last_w, last_batch;
  float conv1a_bound; // max over channels of sum|w1a| + |b1a|: bound on conv1a's outputs for |image| <= 1 (fp16x3 range guard)
  bool x_is_planes;   // the last extract stored the encoder output as pre-split planes
  bool head_fused;    // the last extract ran convPb + softmax + depth-to-space as one kernel: h->logits is stale
  float* b1_dbg;      // fp32 copy of conv1b's pooled output (dim_sp_debug_conv1b)
  float* x_dbg;       // fp32 copy of it, built on request by dim_sp_debug_buffers
  bool bn;            // dim_spo_create: the encoder layers' bias buffers are [b | s | t] and their convolutions run the BatchNorm epilogue
  // sparse descriptor head (allocated on its first use, like the dense da / dd on theirs): the cells that keypoints sample, compact rows of convDa / convDb
  float *da_rows, *dd_rows;
  int *cell_rows, *n_rows, *row_of_cell;
  int desc_slots;     // rows per image of the last sparse extract; 0: the last extract ran the dense head
};

namespace {
// The sparse descriptor head is chosen when its worst-case row count min(4 capacity, h w) is at most this fraction of the map's cells: the measured
// crossover at 1024^2 (profiles/sp_sparse_desc_ab.json).  Known on the host: no synchronisation.
constexpr double kSparseDescMaxFraction = 0.8;

int sp_alloc_dense_desc(dim_sp* h) {
  const size_t cells = (size_t)h->max_batch * (h->max_h / 8) * (h->max_w / 8);
  if (!h->da) DIM_TRY(dim_dev_alloc(&h->base, &h->da, cells * 256));
  if (!h->dd) DIM_TRY(dim_dev_alloc(&h->base, &h->dd, cells * 256));
  return 0;
}
int sp_alloc_sparse_desc(dim_sp* h) {
  const size_t hw = (size_t)(h->max_h / 8) * (h->max_w / 8), B = h->max_batch;
  const size_t slots = std::min((size_t)4 * h->capacity, hw);
  if (!h->da_rows) DIM_TRY(dim_dev_alloc(&h->base, &h->da_rows, B * slots * 256));
  if (!h->dd_rows) DIM_TRY(dim_dev_alloc(&h->base, &h->dd_rows, B * slots * 256));
  if (!h->cell_rows) DIM_TRY(dim_dev_alloc(&h->base, &h->cell_rows, B * slots));
  if (!h->row_of_cell) DIM_TRY(dim_dev_alloc(&h->base, &h->row_of_cell, B * hw));
  if (!h->n_rows) DIM_TRY(dim_dev_alloc(&h->base, &h->n_rows, B));
  return 0;
}
// the dense descriptor head on the last batch's encoder output (dim_sp_extract's dense path; dim_sp_debug_buffers after a sparse extract)
int sp_dense_desc(dim_sp* h, int batch, int hh, int ww, int pmode, bool planes, unsigned* sat_head, bool prof, hipStream_t s) {
  DIM_TRY(sp_alloc_dense_desc(h));
  if (prof) dim_prof_begin(DIM_PROF_SP_CONVDA, s);
  if (planes) DIM_RUN(launch_conv3x3_x6_planes(h->x, h->wsp[2][10], h->bias[10], h->da, batch, hh, ww, 128, 256, 0, 1, 1, 0, s, sat_head, 0));
  else if (pmode != 0) DIM_RUN(launch_conv3x3_x6(h->x, h->wsp[pmode][10], h->bias[10], h->da, batch, hh, ww, 128, 256, 0, 1, s, sat_head, 0));
  else DIM_RUN(launch_conv3x3(h->x, h->wk[10], h->bias[10], h->da, batch, hh, ww, 128, 256, 0, 1, s));
  if (prof) dim_prof_end(DIM_PROF_SP_CONVDA, s);
  GemmArgs g;
  g.A0 = h->da; g.lda0 = 256; g.B = h->wk[11]; g.ldb = 256; g.bias = h->bias[11];
  g.C = h->dd; g.ldc = 256; g.M = batch * hh * ww; g.N = 256; g.K = 256;
  if (pmode != 0) { g.set_split(h->wsp[pmode][11]); DIM_RUN(launch_gemm_x6(g, 1, s)); }
  else DIM_RUN(launch_gemm(g, 1, s));
  return 0;
}

const int kCin[12] = {1, 64, 64, 64, 64, 128, 128, 128, 128, 256, 128, 256};
const int kCout[12] = {64, 64, 64, 64, 128, 128, 128, 128, 256, 65, 256, 256};
const int kK[12] = {3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 3, 1};

// Both kinds of handle.  bn_st == nullptr: SuperPoint (dim_sp_create).  Otherwise bn_st[l] = s[cout] | t[cout] of encoder layer l (0 .. 7), stored
// behind that layer's bias for the BatchNorm epilogue of conv_x6.hip, and w holds the 1x1 heads with their BatchNorms already folded in.
int sp_create(const dim_sp_weights* w, const std::vector<float>* bn_st, const dim_sp_config* cfg, int max_batch, int max_h, int max_w, int capacity,
              dim_sp** out) {
  DIM_REQUIRE(w && cfg && out, "dim_sp_create: null argument");
  DIM_REQUIRE(max_batch > 0 && max_h >= 8 && max_w >= 8, "dim_sp_create: bad sizes");
  DIM_REQUIRE(cfg->max_keypoints != 0 && cfg->max_keypoints >= -1, "\"max_keypoints\" must be positive or \"-1\"");  // SPN:152-154
  DIM_REQUIRE(capacity > 0 && capacity >= cfg->max_keypoints, "dim_sp_create: capacity %d < max_keypoints %d", capacity, cfg->max_keypoints);
  DIM_REQUIRE(cfg->nms_radius >= 0, "nms_radius must be >= 0");  // SPN:49
  std::unique_ptr<dim_sp, void (*)(dim_sp*)> guard(new dim_sp(), dim_sp_destroy);
  dim_sp* const h = guard.get();
  DimHandleBase* const hb = &h->base;
  memset((void*)&h->cfg, 0, sizeof(h->cfg));
  h->cfg = *cfg;
  h->max_batch = max_batch; h->max_h = max_h; h->max_w = max_w; h->capacity = capacity;
  h->last_h = h->last_w = h->last_batch = 0;
  h->b1_dbg = nullptr; h->x_dbg = nullptr; h->head_fused = false;
  h->da = h->dd = nullptr;   // the dense descriptor maps (3.4 GB at 100 x 1024^2): allocated on the first dense use
  h->da_rows = h->dd_rows = nullptr; h->cell_rows = h->n_rows = h->row_of_cell = nullptr; h->desc_slots = 0;
  h->bn = bn_st != nullptr;
  // ---- weights: OIHW (SPN:128-143) -> [tap][cin][cout] / [cin][cout_padded4] ----
  for (int l = 0; l < 12; ++l) {
    const int ci = kCin[l], co = kCout[l], k = kK[l];
    const int co_pad = (co + 3) & ~3;
    // (checked here for every form below: the conv splits take the OIHW tensor itself)
    if (!dim_all_finite(w->conv_w[l], (size_t)k * k * ci * co) || !dim_all_finite(w->conv_b[l], (size_t)co)) { dim_set_error("dim_sp_create: non-finite value in the weights of layer %d", l); return -1; }
    std::vector<float> host((size_t)k * k * ci * co_pad, 0.0f);
    for (int o = 0; o < co; ++o)
      for (int i = 0; i < ci; ++i)
        for (int t = 0; t < k * k; ++t) host[((size_t)t * ci + i) * co_pad + o] = w->conv_w[l][((size_t)o * ci + i) * k * k + t];
    if (k == 3 && ci >= 64) {
      for (int mode = 1; mode <= 2; ++mode) {
        std::vector<unsigned short> hx(conv_split_weight_elems(ci, co, mode));
        SplitWeights& sw = h->wsp[mode][l];
        prepare_conv_weights_split(w->conv_w[l], ci, co, mode, hx.data(), &sw);
        DIM_TRY(dim_upload_split(hb, &sw, hx, mode, sw.n_pad));
      }
    }
#ifdef DIM_RESEARCH
    if (l == 1) {  // conv1b: the Winograd variant's weights (dim_tune_set key 15; research build)
      std::vector<unsigned short> hx(conv_wino_weight_elems(ci, co));
      SplitWeights& sw = h->wsw[l];
      prepare_conv_weights_wino(w->conv_w[l], ci, co, hx.data(), &sw);
      DIM_TRY(dim_upload_split(hb, &sw, hx, 2, sw.n_pad));
    }
#endif
    if (k == 1) {  // the two 1x1 heads (convPb 256 -> 65, convDb 256 -> 256) run on the split GEMM
      std::vector<float> kn((size_t)ci * co);
      for (int o = 0; o < co; ++o)
        for (int i = 0; i < ci; ++i) kn[(size_t)i * co + o] = w->conv_w[l][(size_t)o * ci + i];
      for (int mode = 1; mode <= 2; ++mode) DIM_TRY(dim_upload_gemm_split(hb, &h->wsp[mode][l], kn.data(), ci, co, (co + 127) / 128 * 128, mode));
    }
    DIM_TRY(dim_upload_f32(hb, &h->wk[l], host));
    std::vector<float> bv(co_pad, 0.0f);
    memcpy(bv.data(), w->conv_b[l], co * sizeof(float));
    if (bn_st && l < 8) bv.insert(bv.end(), bn_st[l].begin(), bn_st[l].end());   // (co_pad == co for these layers)
    DIM_TRY(dim_upload_f32(hb, &h->bias[l], bv));
  }
  h->conv1a_bound = 0.0f;
  for (int o = 0; o < 64; ++o) {
    float sum = fabsf(w->conv_b[0][o]);
    for (int t = 0; t < 9; ++t) sum += fabsf(w->conv_w[0][o * 9 + t]);
    if (bn_st) sum = fabsf(bn_st[0][o]) * sum + fabsf(bn_st[0][64 + o]);  // conv1a's BatchNorm follows its ReLU: |s| bound + |t|
    h->conv1a_bound = fmaxf(h->conv1a_bound, sum);
  }
  // ---- activations ----
  const size_t B = max_batch, H = max_h, W = max_w;
  const size_t H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2, hh = H4 / 2, ww = W4 / 2;
  h->a1 = nullptr;  // conv1a's 64-channel full-resolution map: only the unfused A/B path needs it, allocated on first use
  DIM_TRY(dim_dev_alloc(hb, &h->b1, B * dim_planes_image_pixels(H2, W2) * 64));
  DIM_TRY(dim_dev_alloc(hb, &h->a2, B * dim_planes_image_pixels(H2, W2) * 64));
  DIM_TRY(dim_dev_alloc(hb, &h->b2, B * dim_planes_image_pixels(H4, W4) * 64));
  DIM_TRY(dim_dev_alloc(hb, &h->a3, B * dim_planes_image_pixels(H4, W4) * 128));
  DIM_TRY(dim_dev_alloc(hb, &h->b3, B * dim_planes_image_pixels(hh, ww) * 128));
  DIM_TRY(dim_dev_alloc(hb, &h->a4, B * dim_planes_image_pixels(hh, ww) * 128));
  DIM_TRY(dim_dev_alloc(hb, &h->x, B * dim_planes_image_pixels(hh, ww) * 128));
  DIM_TRY(dim_dev_alloc(hb, &h->pa, B * hh * ww * 256));
  DIM_TRY(dim_dev_alloc(hb, &h->logits, B * hh * ww * 65));
  DIM_TRY(dim_dev_alloc(hb, &h->smap, B * hh * ww * 64));
  DIM_TRY(dim_dev_alloc(hb, &h->nms, B * hh * ww * 64));
  DIM_TRY(dim_dev_alloc(hb, &h->cand_score, B * hh * ww * 64));
  DIM_TRY(dim_dev_alloc(hb, &h->cand_idx, B * hh * ww * 64));
  DIM_TRY(dim_dev_alloc(hb, &h->rowcount, B * hh * 8));
  DIM_TRY(dim_dev_alloc(hb, &h->rowoff, B * hh * 8));
  DIM_TRY(dim_dev_alloc(hb, &h->ncand, B));
  h->topk_keys = nullptr;
  if (topk_scratch_keys(max_batch, cfg->max_keypoints)) DIM_TRY(dim_dev_alloc(hb, &h->topk_keys, topk_scratch_keys(max_batch, cfg->max_keypoints)));
  *out = guard.release();
  return 0;
}
}  // namespace

extern "C" {

void dim_sp_destroy(dim_sp* h) {
  if (!h) return;
  dim_handle_release(&h->base);
  delete h;
}

int dim_sp_create(const dim_sp_weights* w, const dim_sp_config* cfg, int max_batch, int max_h, int max_w, int capacity,
                  dim_sp** out) {
  return sp_create(w, nullptr, cfg, max_batch, max_h, max_w, capacity, out);
}

int dim_spo_create(const dim_spo_weights* w, const dim_sp_config* cfg, int max_batch, int max_h, int max_w, int capacity, dim_sp** out) {
  DIM_REQUIRE(w && cfg && out, "dim_spo_create: null argument");
  DIM_REQUIRE(isfinite(w->bn_eps), "dim_spo_create: bn_eps is not finite");
  // s = gamma / sqrt(var + eps), t = beta - mean s, in double
  std::vector<double> s[12], t[12];
  for (int l = 0; l < 12; ++l) {
    const int ci = kCin[l], co = kCout[l], k = kK[l];
    DIM_REQUIRE(w->conv_w[l] && w->conv_b[l] && w->bn_gamma[l] && w->bn_beta[l] && w->bn_mean[l] && w->bn_var[l], "dim_spo_create: null tensor in layer %d", l);
    if (!dim_all_finite(w->conv_w[l], (size_t)k * k * ci * co) || !dim_all_finite(w->conv_b[l], (size_t)co) || !dim_all_finite(w->bn_gamma[l], (size_t)co) ||
        !dim_all_finite(w->bn_beta[l], (size_t)co) || !dim_all_finite(w->bn_mean[l], (size_t)co) || !dim_all_finite(w->bn_var[l], (size_t)co)) {
      dim_set_error("dim_spo_create: non-finite value in the weights of layer %d", l);
      return -1;
    }
    s[l].resize(co); t[l].resize(co);
    for (int o = 0; o < co; ++o) {
      const double v = (double)w->bn_var[l][o] + w->bn_eps;
      DIM_REQUIRE(v > 0.0, "dim_spo_create: running_var + eps = %g <= 0 in layer %d, channel %d", v, l, o);
      s[l][o] = (double)w->bn_gamma[l][o] / sqrt(v);
      t[l][o] = (double)w->bn_beta[l][o] - (double)w->bn_mean[l][o] * s[l][o];
      DIM_REQUIRE(isfinite((float)s[l][o]) && isfinite((float)t[l][o]), "dim_spo_create: BatchNorm of layer %d, channel %d is not finite in fp32", l, o);
    }
  }
  std::vector<float> st[8];
  for (int l = 0; l < 8; ++l) {
    const int co = kCout[l];
    st[l].resize(2 * (size_t)co);
    for (int o = 0; o < co; ++o) { st[l][o] = (float)s[l][o]; st[l][co + o] = (float)t[l][o]; }
  }
  // The heads: a = relu(conv3x3(x) + b) keeps the plain epilogue; z = s_a a + t_a, u = W z + b, out = s_b u + t_b is the 1x1 convolution
  // W'[o][i] = s_b[o] W[o][i] s_a[i], b'[o] = s_b[o] (b[o] + sum_i W[o][i] t_a[i]) + t_b[o] — a 1x1 convolution has no padding: exact.
  dim_sp_weights f;
  std::vector<float> fw[2], fb[2];
  for (int l = 0; l < 12; ++l) { f.conv_w[l] = w->conv_w[l]; f.conv_b[l] = w->conv_b[l]; }
  for (int hd = 0; hd < 2; ++hd) {
    const int la = 8 + 2 * hd, lb = la + 1, ci = kCin[lb], co = kCout[lb];
    fw[hd].resize((size_t)co * ci); fb[hd].resize(co);
    for (int o = 0; o < co; ++o) {
      double acc = (double)w->conv_b[lb][o];
      for (int i = 0; i < ci; ++i) {
        const double wv = (double)w->conv_w[lb][(size_t)o * ci + i];
        acc += wv * t[la][i];
        fw[hd][(size_t)o * ci + i] = (float)(s[lb][o] * wv * s[la][i]);
      }
      fb[hd][o] = (float)(s[lb][o] * acc + t[lb][o]);
    }
    f.conv_w[lb] = fw[hd].data(); f.conv_b[lb] = fb[hd].data();
  }
  dim_sp_config c = *cfg;
  c.fix_sampling = 1;   // the open network's one sampler (superpoint_pytorch.py sample_descriptors)
  return sp_create(&f, st, &c, max_batch, max_h, max_w, capacity, out);
}

int dim_sp_extract(dim_sp* h, const float* images_dev, int batch, int H, int W, float* kpts_xy_dev, float* scores_dev,
                   float* desc_dev, int32_t* n_kpts_dev, void* stream) {
  DIM_REQUIRE(h && images_dev && kpts_xy_dev && scores_dev && desc_dev && n_kpts_dev, "dim_sp_extract: null argument");
  DimTuneScope tune_scope(&h->base);
  DIM_REQUIRE(batch >= 1 && batch <= h->max_batch, "dim_sp_extract: batch %d outside [1,%d]", batch, h->max_batch);
  DIM_REQUIRE(H >= 8 && W >= 8 && H <= h->max_h && W <= h->max_w && (size_t)H * W <= (size_t)h->max_h * h->max_w,
              "dim_sp_extract: image %dx%d outside the handle's %dx%d", H, W, h->max_h, h->max_w);
  hipStream_t s = (hipStream_t)stream;
  const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2, hh = H4 / 2, ww = W4 / 2;  // floor at every pool (Q12)
  const int H8 = hh * 8, W8 = ww * 8;
#define SP_SITE(id, x) do { dim_prof_begin(id, s); DIM_RUN(x); dim_prof_end(id, s); } while (0)
  const int pmode = dim_precision_mode();  // 2 (default) fp16x3 / 1 bf16x6: fp32-accurate products on the 16-bit matrix cores; 0: fp32 MFMA
  const bool x6 = pmode != 0;
  const int bn = h->bn ? 1 : 0;
  DIM_REQUIRE(!bn || (x6 && dim_fuse_conv1a() && !(dim_conv_winograd() & 1)),
              "dim_sp_extract: an open-SuperPoint handle (dim_spo_create) runs in fp16x3 / bf16x6 with the fused conv1a only (dim_tune_set keys 1, 3, 15)");
  // fp16x3 range guard (dim_common.h): producers of values that a later split consumes report max|x| > 4094
  unsigned* sat_enc = pmode == 2 ? dim_sat_counter(DIM_SAT_SP_ENCODER) : nullptr;
  unsigned* sat_head = pmode == 2 ? dim_sat_counter(DIM_SAT_SP_HEADS) : nullptr;
  unsigned* sat_img = pmode == 2 ? dim_sat_counter(DIM_SAT_SP_IMAGE) : nullptr;
  if (pmode == 2 && !(h->conv1a_bound <= DIM_F16_ACT_LIMIT)) dim_sat_host_bump(DIM_SAT_SP_IMAGE);  // conv1a's outputs may leave the range
  auto conv = [&](int l, const float* in, float* out, int Hh, int Ww, int ci, int co, int pool) -> int {
    return x6 ? launch_conv3x3_x6(in, h->wsp[pmode][l], h->bias[l], out, batch, Hh, Ww, ci, co, pool, 1, s, l >= 8 ? sat_head : sat_enc, l < 8 ? bn : 0)
              : launch_conv3x3(in, h->wk[l], h->bias[l], out, batch, Hh, Ww, ci, co, pool, 1, s);
  };
  // encoder (SPN:161-171)
  // fp16x3 + fused conv1a: the conv-to-conv activations b1 .. a4 are stored as pre-split fp16 planes (conv_x6.hip PIN / POUT):
  // each value is split once by its producer instead of ~1.3 x (cout / 64) times by its consumers
  const bool planes = pmode == 2 && dim_fuse_conv1a() && dim_presplit_activations();
  auto convp = [&](int l, const float* in, float* out, int Hh, int Ww, int ci, int co, int pool, int pin, int pout) -> int {
    return launch_conv3x3_x6_planes(in, h->wsp[2][l], h->bias[l], out, batch, Hh, Ww, ci, co, pool, 1, pin, pout, s, l >= 8 ? sat_head : sat_enc, l < 8 ? bn : 0);
  };
#ifdef DIM_RESEARCH
  if (pmode == 2 && dim_fuse_conv1a() && (dim_conv_winograd() & 1)) {  // Winograd F(2,3) along x: 2/3 of the MFMAs (conv_wg.hip)
    // the transformed activations reach 2 x conv1a's output bound: check the doubled bound on the host as the direct path checks the plain one
    if (!(2.0f * h->conv1a_bound <= DIM_F16_ACT_LIMIT)) dim_sat_host_bump(DIM_SAT_SP_IMAGE);
    SP_SITE(DIM_PROF_SP_CONV1B, launch_conv3x3_wg_fused1a(images_dev, h->wk[0], h->bias[0], h->wsw[1], h->bias[1], h->b1, batch, H, W, 64, 1, planes ? 1 : 0, s, sat_enc, sat_img));
  } else
#endif
  if (x6 && dim_fuse_conv1a()) {  // conv1a evaluated inside conv1b's halo staging: its 64-channel full-resolution map never exists
    SP_SITE(DIM_PROF_SP_CONV1B, launch_conv3x3_x6_fused1a(images_dev, h->wk[0], h->bias[0], h->wsp[pmode][1], h->bias[1], h->b1, batch, H, W, 64, 1, 1, planes ? 1 : 0, s, sat_enc, sat_img, bn));
  } else {
    if (!h->a1) DIM_RUN(dim_dev_alloc(&h->base, &h->a1, (size_t)h->max_batch * h->max_h * h->max_w * 64));
    SP_SITE(DIM_PROF_SP_CONV1A, launch_conv1a(images_dev, h->wk[0], h->bias[0], h->a1, batch, H, W, s));
    SP_SITE(DIM_PROF_SP_CONV1B, conv(1, h->a1, h->b1, H, W, 64, 64, 1));
  }
  if (planes) {
    SP_SITE(DIM_PROF_SP_CONV2A, convp(2, h->b1, h->a2, H2, W2, 64, 64, 0, 1, 1));
    SP_SITE(DIM_PROF_SP_CONV2B, convp(3, h->a2, h->b2, H2, W2, 64, 64, 1, 1, 1));
    SP_SITE(DIM_PROF_SP_CONV3A, convp(4, h->b2, h->a3, H4, W4, 64, 128, 0, 1, 1));
    SP_SITE(DIM_PROF_SP_CONV3B, convp(5, h->a3, h->b3, H4, W4, 128, 128, 1, 1, 1));
    SP_SITE(DIM_PROF_SP_CONV4A, convp(6, h->b3, h->a4, hh, ww, 128, 128, 0, 1, 1));
    SP_SITE(DIM_PROF_SP_CONV4B, convp(7, h->a4, h->x, hh, ww, 128, 128, 0, 1, 1));  // the encoder output feeds 8 cout blocks of the two heads
  } else {
    SP_SITE(DIM_PROF_SP_CONV2A, conv(2, h->b1, h->a2, H2, W2, 64, 64, 0));
    SP_SITE(DIM_PROF_SP_CONV2B, conv(3, h->a2, h->b2, H2, W2, 64, 64, 1));
    SP_SITE(DIM_PROF_SP_CONV3A, conv(4, h->b2, h->a3, H4, W4, 64, 128, 0));
    SP_SITE(DIM_PROF_SP_CONV3B, conv(5, h->a3, h->b3, H4, W4, 128, 128, 1));
    SP_SITE(DIM_PROF_SP_CONV4A, conv(6, h->b3, h->a4, hh, ww, 128, 128, 0));
    SP_SITE(DIM_PROF_SP_CONV4B, conv(7, h->a4, h->x, hh, ww, 128, 128, 0));
  }
  // detector head (SPN:174-180)
  h->x_is_planes = planes;
  if (planes) SP_SITE(DIM_PROF_SP_CONVPA, convp(8, h->x, h->pa, hh, ww, 128, 256, 0, 1, 0));
  else SP_SITE(DIM_PROF_SP_CONVPA, conv(8, h->x, h->pa, hh, ww, 128, 256, 0));
  {
    GemmArgs g;
    g.A0 = h->pa; g.lda0 = 256; g.B = h->wk[9]; g.ldb = 68; g.bias = h->bias[9];
    g.C = h->logits; g.ldc = 65; g.M = batch * hh * ww; g.N = 65; g.K = 256;
    // fp16x3: convPb + softmax + depth-to-space in one kernel (gemm_x6_head_kernel): the logits are not stored (dim_sp_debug_buffers rebuilds them)
    h->head_fused = pmode == 2 && dim_fuse_sp_head();
    if (h->head_fused) {
      g.set_split(h->wsp[pmode][9]); g.d2s_out = h->smap; g.d2s_h = hh; g.d2s_w = ww;
      DIM_RUN(launch_gemm_x6(g, 1, s));
    } else {
      if (x6) { g.set_split(h->wsp[pmode][9]); DIM_RUN(launch_gemm_x6(g, 1, s)); }
      else DIM_RUN(launch_gemm(g, 1, s));
      DIM_RUN(launch_softmax_d2s(h->logits, h->smap, batch, hh, ww, s));
    }
  }
  DIM_RUN(launch_nms(h->smap, h->nms, batch, H8, W8, h->cfg.nms_radius, s));
  // selection (SPN:183-210)
  DIM_RUN(launch_select(h->nms, batch, H8, W8, h->cfg.keypoint_threshold, h->cfg.remove_borders, h->rowcount, h->rowoff,
                       h->ncand, h->cand_score, h->cand_idx, s));
  DIM_RUN(launch_topk(h->cand_score, h->cand_idx, h->ncand, batch, H8, W8, h->cfg.max_keypoints, h->capacity, kpts_xy_dev,
                     scores_dev, n_kpts_dev, h->topk_keys, 0, s));
  // descriptor head (SPN:213-221).  The keypoints are known: with few enough of them convDa / convDb run only on the cells that the sampler will
  // read (at most four per keypoint), listed on the device in raster order; per cell the arithmetic is the dense path's, bit for bit.  The sparse
  // form exists for the pre-split fp16x3 encoder output; keep-all handles (max_keypoints = -1) and everything else stay dense.
  const int slots = (int)std::min((size_t)4 * h->capacity, (size_t)hh * ww);
  const int sparse_sel = dim_sparse_desc();
  const bool sparse = planes && (sparse_sel == 2 || (sparse_sel == 1 && h->cfg.max_keypoints > 0 && (double)slots <= kSparseDescMaxFraction * (double)hh * ww));
  if (sparse) {
    DIM_RUN(sp_alloc_sparse_desc(h));
    DIM_RUN(launch_desc_cell_list(kpts_xy_dev, n_kpts_dev, batch, hh, ww, h->capacity, h->cfg.fix_sampling, slots, h->row_of_cell, h->cell_rows, h->n_rows, s));
    SP_SITE(DIM_PROF_SP_CONVDA, launch_conv3x3_x6_rows(h->x, h->wsp[2][10], h->bias[10], h->da_rows, batch, hh, ww, 128, 256, 1, h->cell_rows, h->n_rows, slots, s, sat_head));
    GemmArgs g;
    g.A0 = h->da_rows; g.lda0 = 256; g.strideA0 = (long long)slots * 256; g.B = h->wk[11]; g.ldb = 256; g.bias = h->bias[11];
    g.C = h->dd_rows; g.ldc = 256; g.strideC = (long long)slots * 256; g.M = slots; g.N = 256; g.K = 256; g.rows = h->n_rows;
    g.set_split(h->wsp[2][11]);
    DIM_RUN(launch_gemm_x6(g, batch, s));
    DIM_RUN(launch_sample_desc(h->dd_rows, kpts_xy_dev, n_kpts_dev, desc_dev, batch, hh, ww, h->capacity, h->cfg.fix_sampling, s, h->row_of_cell, slots));
  } else {
    DIM_RUN(sp_dense_desc(h, batch, hh, ww, pmode, planes, sat_head, true, s));
    DIM_RUN(launch_sample_desc(h->dd, kpts_xy_dev, n_kpts_dev, desc_dev, batch, hh, ww, h->capacity, h->cfg.fix_sampling, s));
  }
  h->desc_slots = sparse ? slots : 0;
#undef SP_SITE
  h->last_h = hh; h->last_w = ww; h->last_batch = batch;
  return 0;
}

int dim_sp_debug_buffers(dim_sp* h, const float** encoder, const float** logits, const float** score_map,
                         const float** nms_map, const float** dense_desc, int* h8, int* w8) {
  DIM_REQUIRE(h, "dim_sp_debug_buffers: null handle");
  DimTuneScope tune_scope(&h->base);
  if (encoder) {
    *encoder = h->x;
    if (h->x_is_planes) {  // rebuild fp32 from the planes of the last batch
      if (!h->x_dbg && dim_dev_alloc(&h->base, &h->x_dbg, (size_t)h->max_batch * (h->max_h / 8) * (h->max_w / 8) * 128) != 0) return -1;
      if (launch_planes_to_f32(h->x, h->last_batch, h->last_h * h->last_w, 128, h->x_dbg, nullptr) != 0) return -1;
      DIM_HIP(hipDeviceSynchronize());
      *encoder = h->x_dbg;
    }
  }
  if (logits) {
    if (h->head_fused && h->last_batch > 0) {   // the fused detector tail never stores the logits: rebuild them with the plain GEMM on the last batch's convPa output
      GemmArgs g;
      g.A0 = h->pa; g.lda0 = 256; g.B = h->wk[9]; g.ldb = 68; g.bias = h->bias[9];
      g.C = h->logits; g.ldc = 65; g.M = h->last_batch * h->last_h * h->last_w; g.N = 65; g.K = 256;
      g.set_split(h->wsp[2][9]);
      if (launch_gemm_x6(g, 1, nullptr) != 0) return -1;
      DIM_HIP(hipDeviceSynchronize());
    }
    *logits = h->logits;
  }
  if (score_map) *score_map = h->smap;
  if (nms_map) *nms_map = h->nms;
  if (dense_desc) {
    if (h->desc_slots > 0 && h->last_batch > 0) {   // the sparse head stored only the sampled cells: rebuild the dense map from the last batch's encoder output
      if (sp_dense_desc(h, h->last_batch, h->last_h, h->last_w, 2, true, nullptr, false, nullptr) != 0) return -1;
      DIM_HIP(hipDeviceSynchronize());
    } else if (sp_alloc_dense_desc(h) != 0) return -1;
    *dense_desc = h->dd;
  }
  if (h8) *h8 = h->last_h * 8;
  if (w8) *w8 = h->last_w * 8;
  return 0;
}

int dim_sp_debug_conv1b(dim_sp* h, int batch, int H, int W, const float** out_f32, int* h2, int* w2) {
  // fp32 NHWC copy [batch][H/2][W/2][64] of conv1b's pooled output of the last extract (A/B of the convolution variants)
  DIM_REQUIRE(h && out_f32 && batch >= 1 && batch <= h->max_batch, "dim_sp_debug_conv1b: bad argument");
  DimTuneScope tune_scope(&h->base);
  const int H2 = H / 2, W2 = W / 2;
  if (!h->b1_dbg && dim_dev_alloc(&h->base, &h->b1_dbg, (size_t)h->max_batch * (h->max_h / 2) * (h->max_w / 2) * 64) != 0) return -1;
  const bool planes = h->x_is_planes;   // how the last extract stored b1 .. x (a guarded call may have re-run in another arithmetic than the current one)
  if (planes) {
    if (launch_planes_to_f32(h->b1, batch, H2 * W2, 64, h->b1_dbg, nullptr) != 0) return -1;
  } else {
    DIM_HIP(hipMemcpy(h->b1_dbg, h->b1, (size_t)batch * H2 * W2 * 64 * sizeof(float), hipMemcpyDeviceToDevice));
  }
  DIM_HIP(hipDeviceSynchronize());
  *out_f32 = h->b1_dbg;
  if (h2) *h2 = H2;
  if (w2) *w2 = W2;
  return 0;
}

int dim_sp_desc_rows(dim_sp* h, const int32_t** n_rows_dev, int* slots) {
  DIM_REQUIRE(h && slots, "dim_sp_desc_rows: null argument");
  *slots = h->desc_slots;
  if (n_rows_dev) *n_rows_dev = h->desc_slots > 0 ? h->n_rows : nullptr;
  return 0;
}

int dim_sp_candidate_counts(dim_sp* h, const int32_t** ncand_dev) {
  DIM_REQUIRE(h && ncand_dev, "dim_sp_candidate_counts: null argument");
  *ncand_dev = h->ncand;
  return 0;
}

}  // extern "C"
