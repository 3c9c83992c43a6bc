// dim_xfeat_* : resident XFeat extractor (C ABI in include/dim_hip.h).
// Replaces XFeat.detectAndCompute (thirdparty/accelerated_features/modules/xfeat.py:50-103 = XFM) over XFeatModel.forward (modules/model.py:123-154 =
// XFN) and InterpolateSparse2d (modules/interpolator.py = XFI) as driven by XFeatExtractor (extractors/xfeat.py): top_k from the config, the
// detection threshold the network's own.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/dim_hip.h"
#include "nhwc_conv.h"
#include "sp_kernels.h"
#include "xfeat_kernels.h"

namespace {
// XFN:43-92 in weights.py's XFEAT_BASIC order: cout, cin, kernel, stride
struct XfGeo { int co, ci, k, stride; };
constexpr int XF_NB = 23;
const XfGeo XF_BASIC[XF_NB] = {
    {4, 1, 3, 1}, {8, 4, 3, 2}, {8, 8, 3, 1}, {24, 8, 3, 2},                      // block1 (the stem kernels)
    {24, 24, 3, 1}, {24, 24, 3, 1},                                               // block2
    {64, 24, 3, 2}, {64, 64, 3, 1}, {64, 64, 1, 1},                               // block3
    {64, 64, 3, 2}, {64, 64, 3, 1}, {64, 64, 3, 1},                               // block4
    {128, 64, 3, 2}, {128, 128, 3, 1}, {128, 128, 3, 1}, {64, 128, 1, 1},         // block5
    {64, 64, 3, 1}, {64, 64, 3, 1},                                               // block_fusion.0 / .1
    {64, 64, 1, 1}, {64, 64, 1, 1},                                               // heatmap_head.0 / .1
    {64, 64, 1, 1}, {64, 64, 1, 1}, {64, 64, 1, 1},                               // keypoint_head.0 / .1 / .2
};
enum { XF_L_BLOCK2 = 4, XF_L_BLOCK3 = 6, XF_L_BLOCK4 = 9, XF_L_BLOCK5 = 12, XF_L_FUSION = 16, XF_L_HEAT = 18, XF_L_KP = 20 };

// byte offsets of dim_op_xfeat_select's workspace
struct XfSelectWs { size_t key, rowcount, rowoff, ncand, cand_score, cand_idx, keys, total; };
XfSelectWs xf_select_ws(int batch, int H, int W, int k) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t rows = (size_t)batch * H, px = rows * W;
  XfSelectWs w;
  w.key = 0;
  w.rowcount = w.key + up(px * 4);
  w.rowoff = w.rowcount + up(rows * 4);
  w.ncand = w.rowoff + up(rows * 4);
  w.cand_score = w.ncand + up((size_t)batch * 4);
  w.cand_idx = w.cand_score + up(px * 4);
  w.keys = w.cand_idx + up(px * 4);
  w.total = w.keys + up(topk_scratch_keys(batch, k) * 8);
  return w;
}

// NMS -> key -> select -> sort (XFM:74-87): the library's chain on the key map, always sorted; kpts_px (x, y) pixel positions, scores = keys
int xf_select_chain(const float* k1h, const float* h1, float* key, float thr, int top_k, int capacity, int batch, int H, int W, int* rowcount, int* rowoff, int* ncand,
                    float* cand_score, int* cand_idx, unsigned long long* topk_keys, float* kpts_px, float* scores, int* n_out, hipStream_t s) {
  int rc = launch_xf_keys(k1h, h1, key, thr, batch, H, W, s);
  if (rc != 0) return rc;
  rc = launch_select_ex(key, batch, H, W, 0.f, nullptr, 0, rowcount, rowoff, ncand, cand_score, cand_idx, 0, s);
  if (rc != 0) return rc;
  return launch_topk(cand_score, cand_idx, ncand, batch, H, W, top_k, capacity, kpts_px, scores, n_out, topk_keys, 1, s);
}
}  // namespace

struct dim_xfeat {
  DimHandleBase base;   // first member: dim_handle_tune_set
  dim_xfeat_config cfg;
  int max_batch, max_h, max_w, capacity, stride;
  XfStem stem;
  NhwcConvLayer L[XF_NB], fusion2;   // L[0..3] unused (stem); fusion2 = block_fusion.2 (1x1 with bias, no activation)
  float *heat_w, *heat_b, *kp_w, *kp_b;
  float *norm, *a2, *b2, *q0, *q1, *q2, *e[5], *f[3], *g[3], *g3, *h1, *k1h, *key;
  double *partial, *stats;
  float *cand_score, *kpts_px;
  int *cand_idx, *rowcount, *rowoff, *ncand;
  unsigned long long* topk_keys;
  int last_h, last_w;
};

extern "C" {

void dim_xfeat_destroy(dim_xfeat* h) {
  if (!h) return;
  dim_handle_release(&h->base);
  delete h;
}

int dim_xfeat_create(const dim_xfeat_weights* w, const dim_xfeat_config* cfg, int max_batch, int max_h, int max_w, int capacity, dim_xfeat** out) {
  DIM_REQUIRE(w && cfg && out, "dim_xfeat_create: null argument");
  const int stride = cfg->desc_stride == 0 ? 64 : cfg->desc_stride;
  DIM_REQUIRE(stride >= 64 && stride % 4 == 0 && stride <= 128, "dim_xfeat_create: desc_stride %d must be 0 or a multiple of 4 in [64, 128]", cfg->desc_stride);
  DIM_REQUIRE(capacity > 0 && capacity <= 32768, "dim_xfeat_create: capacity %d outside [1, 32768]", capacity);
  DIM_REQUIRE(cfg->top_k > 0 && cfg->top_k <= capacity, "dim_xfeat_create: capacity %d must cover top_k %d", capacity, cfg->top_k);
  DIM_REQUIRE(max_batch > 0 && max_batch <= 64, "dim_xfeat_create: max_batch %d outside [1, 64]", max_batch);
  DIM_REQUIRE(max_h >= 32 && max_w >= 32, "dim_xfeat_create: max_h %d / max_w %d below 32 (the frame is resized DOWN to multiples of 32, XFM:236)", max_h, max_w);
  DIM_REQUIRE((long long)max_batch * max_h * max_w <= 0x7fffffffLL, "dim_xfeat_create: %d images of %d x %d exceed 2^31 pixels", max_batch, max_h, max_w);
  DIM_REQUIRE(cfg->detection_threshold >= 0.f && cfg->detection_threshold < 1.f, "dim_xfeat_create: detection_threshold %g outside [0, 1)", (double)cfg->detection_threshold);
  std::unique_ptr<dim_xfeat, void (*)(dim_xfeat*)> guard(new dim_xfeat(), dim_xfeat_destroy);
  dim_xfeat* const h = guard.get();
  DimHandleBase* const hb = &h->base;
  h->cfg = *cfg; h->stride = stride;
  h->max_batch = max_batch; h->max_h = max_h; h->max_w = max_w; h->capacity = capacity;
  h->last_h = h->last_w = 0;

  // BasicLayer (XFN:12-25): BatchNorm2d(affine=False) in eval mode between convolution and ReLU, folded in fp64: w' = w * sc, bias = -running_mean * sc
  // with sc = 1 / sqrt(running_var + 1e-5)
  std::vector<double> sc[XF_NB], bi[XF_NB];
  for (int i = 0; i < XF_NB; ++i) {
    const XfGeo& g = XF_BASIC[i];
    DIM_REQUIRE(w->basic_w[i] && w->basic_mean[i] && w->basic_var[i], "dim_xfeat_create: BasicLayer %d has a null tensor", i);
    DIM_REQUIRE(dim_all_finite(w->basic_w[i], (size_t)g.co * g.ci * g.k * g.k) && dim_all_finite(w->basic_mean[i], g.co) && dim_all_finite(w->basic_var[i], g.co),
                "dim_xfeat_create: BasicLayer %d holds a non-finite value", i);
    sc[i].resize(g.co); bi[i].resize(g.co);
    for (int c = 0; c < g.co; ++c) {
      DIM_REQUIRE(w->basic_var[i][c] >= 0.0f, "dim_xfeat_create: BasicLayer %d has a negative running_var", i);
      sc[i][c] = 1.0 / sqrt((double)w->basic_var[i][c] + 1e-5);
      bi[i][c] = -(double)w->basic_mean[i][c] * sc[i][c];
    }
  }
  DIM_REQUIRE(w->skip_w && w->skip_b && w->fusion_w && w->fusion_b && w->heat_w && w->heat_b && w->kp_w && w->kp_b, "dim_xfeat_create: a biased 1x1 convolution is null");
  {  // stem: [ci * 9 + tap][co] operands (block1.0: [co][tap])
    auto fold = [&](int i, bool co_major) {
      const XfGeo& g = XF_BASIC[i];
      std::vector<float> o((size_t)g.co * g.ci * 9);
      for (int co = 0; co < g.co; ++co)
        for (int ci = 0; ci < g.ci; ++ci)
          for (int t = 0; t < 9; ++t) {
            const float v = (float)((double)w->basic_w[i][((size_t)co * g.ci + ci) * 9 + t] * sc[i][co]);
            if (co_major) o[(size_t)co * 9 + t] = v; else o[((size_t)ci * 9 + t) * g.co + co] = v;
          }
      return o;
    };
    auto biasv = [&](int i) { std::vector<float> o(XF_BASIC[i].co); for (int c = 0; c < XF_BASIC[i].co; ++c) o[c] = (float)bi[i][c]; return o; };
    float* p[10];
    DIM_TRY(dim_upload_f32(hb, &p[0], fold(0, true))); DIM_TRY(dim_upload_f32(hb, &p[1], biasv(0)));
    DIM_TRY(dim_upload_f32(hb, &p[2], fold(1, false))); DIM_TRY(dim_upload_f32(hb, &p[3], biasv(1)));
    DIM_TRY(dim_upload_f32(hb, &p[4], fold(2, false))); DIM_TRY(dim_upload_f32(hb, &p[5], biasv(2)));
    DIM_TRY(dim_upload_f32(hb, &p[6], fold(3, false))); DIM_TRY(dim_upload_f32(hb, &p[7], biasv(3)));
    DIM_TRY(dim_upload_f32(hb, &p[8], w->skip_w, 24)); DIM_TRY(dim_upload_f32(hb, &p[9], w->skip_b, 24));
    h->stem = XfStem{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]};
  }
  // trunk: [K = taps * cin_pad][N] operands
  auto upload = [&](NhwcConvLayer& L, const float* wt, int co, int ci, int k, int strd, const std::vector<double>* scale, const std::vector<float>& bias, int relu) -> int {
    L.taps = k * k; L.stride = strd; L.relu = relu; L.cin_pad = dim_pad16(ci);
    const int K = L.taps * L.cin_pad;
    std::vector<float> kn((size_t)K * co, 0.0f);
    nhwc_conv_pack_oihw(kn, co, 0, wt, co, ci, k, L.cin_pad, scale);
    return nhwc_conv_upload(hb, &L, kn, K, co, bias);
  };
  for (int i = XF_L_BLOCK2; i < XF_NB; ++i) {
    const XfGeo& g = XF_BASIC[i];
    std::vector<float> bias(g.co);
    for (int c = 0; c < g.co; ++c) bias[c] = (float)bi[i][c];
    DIM_TRY(upload(h->L[i], w->basic_w[i], g.co, g.ci, g.k, g.stride, &sc[i], bias, 1));
  }
  DIM_REQUIRE(dim_all_finite(w->fusion_b, 64), "dim_xfeat_create: block_fusion.2.bias holds a non-finite value");
  DIM_TRY(upload(h->fusion2, w->fusion_w, 64, 64, 1, 1, nullptr, std::vector<float>(w->fusion_b, w->fusion_b + 64), 0));
  DIM_TRY(dim_upload_f32(hb, &h->heat_w, w->heat_w, 64)); DIM_TRY(dim_upload_f32(hb, &h->heat_b, w->heat_b, 1));
  DIM_TRY(dim_upload_f32(hb, &h->kp_w, w->kp_w, 65 * 64)); DIM_TRY(dim_upload_f32(hb, &h->kp_b, w->kp_b, 65));

  const size_t B = max_batch, Hm = (size_t)max_h / 32 * 32, Wm = (size_t)max_w / 32 * 32, NP = Hm * Wm, cap = capacity;
  DIM_TRY(dim_dev_alloc(hb, &h->norm, B * NP)); DIM_TRY(dim_dev_alloc(hb, &h->k1h, B * NP)); DIM_TRY(dim_dev_alloc(hb, &h->key, B * NP));
  DIM_TRY(dim_dev_alloc(hb, &h->partial, B * xf_prep_blocks((int)Hm, (int)Wm) * 2)); DIM_TRY(dim_dev_alloc(hb, &h->stats, B * 2));
  DIM_TRY(dim_dev_alloc(hb, &h->a2, B * NP / 4 * 8)); DIM_TRY(dim_dev_alloc(hb, &h->b2, B * NP / 4 * 8));
  DIM_TRY(dim_dev_alloc(hb, &h->q0, B * NP / 16 * 32)); DIM_TRY(dim_dev_alloc(hb, &h->q1, B * NP / 16 * 32)); DIM_TRY(dim_dev_alloc(hb, &h->q2, B * NP / 16 * 32));
  for (int i = 0; i < 5; ++i) DIM_TRY(dim_dev_alloc(hb, &h->e[i], B * NP / 64 * 64));
  for (int i = 0; i < 3; ++i) DIM_TRY(dim_dev_alloc(hb, &h->f[i], B * NP / 256 * 64));
  for (int i = 0; i < 3; ++i) DIM_TRY(dim_dev_alloc(hb, &h->g[i], B * NP / 1024 * 128));
  DIM_TRY(dim_dev_alloc(hb, &h->g3, B * NP / 1024 * 64)); DIM_TRY(dim_dev_alloc(hb, &h->h1, B * NP / 64));
  DIM_TRY(dim_dev_alloc(hb, &h->cand_score, B * NP)); DIM_TRY(dim_dev_alloc(hb, &h->cand_idx, B * NP)); DIM_TRY(dim_dev_alloc(hb, &h->rowcount, B * Hm));
  DIM_TRY(dim_dev_alloc(hb, &h->rowoff, B * Hm)); DIM_TRY(dim_dev_alloc(hb, &h->ncand, B)); DIM_TRY(dim_dev_alloc(hb, &h->kpts_px, B * cap * 2));
  h->topk_keys = nullptr;
  if (topk_scratch_keys(max_batch, cfg->top_k)) DIM_TRY(dim_dev_alloc(hb, &h->topk_keys, topk_scratch_keys(max_batch, cfg->top_k)));
  *out = guard.release();
  return 0;
}

int dim_xfeat_extract(dim_xfeat* h, const float* images_dev, int batch, int H, int W, int channels, float* kpts_xy_dev, float* scores_dev, float* desc_dev,
                      int32_t* n_kpts_dev, void* stream) {
  DIM_REQUIRE(h && images_dev && kpts_xy_dev && scores_dev && desc_dev && n_kpts_dev, "dim_xfeat_extract: null argument");
  DimTuneScope tune_scope(&h->base);
  DIM_REQUIRE(batch >= 1 && batch <= h->max_batch, "dim_xfeat_extract: batch %d outside [1,%d]", batch, h->max_batch);
  DIM_REQUIRE(channels == 1 || channels == 3, "dim_xfeat_extract: channels %d (1 or 3)", channels);
  DIM_REQUIRE(H >= 32 && W >= 32 && H <= h->max_h && W <= h->max_w, "dim_xfeat_extract: image %dx%d outside [32x32, the handle's %dx%d]", H, W, h->max_h, h->max_w);
  hipStream_t s = (hipStream_t)stream;
  const int Hr = H / 32 * 32, Wr = W / 32 * 32;   // the resized frame (XFM:236)
  const float rh = (float)((double)H / (double)Hr), rw = (float)((double)W / (double)Wr);
  const int H2 = Hr / 2, W2 = Wr / 2, H4 = Hr / 4, W4 = Wr / 4, H8 = Hr / 8, W8 = Wr / 8, H16 = Hr / 16, W16 = Wr / 16, H32 = Hr / 32, W32 = Wr / 32;
  const bool x3 = dim_precision_mode() == 2;   // fp16x3 on the matrix cores; every other mode runs the fp32 MFMA form
  unsigned* const sat = x3 ? dim_sat_counter(DIM_SAT_XFEAT) : nullptr;
  auto conv = [&](const NhwcConvLayer& L, const float* in, int in_h, int in_w, float* out, int Ho, int Wo, bool unfold) -> int {
    NhwcConv a;
    a.in = in; a.cin_pad = L.cin_pad; a.taps = L.taps; a.stride = L.stride; a.in_h = in_h; a.in_w = in_w; a.unfold8 = unfold ? 1 : 0;
    a.wx = &L.wx; a.w32 = L.w32; a.bias = L.bias; a.n_pad = L.n_pad; a.out = out; a.out_c = L.out_c; a.relu = L.relu;
    a.batch = batch; a.H = Ho; a.W = Wo; a.sat = sat;
    return launch_nhwc_conv(a, x3, s);
  };
  // preparation: resize + channel mean, fp64 statistics in two fixed-order stages, InstanceNorm (XFM:219-240, XFN:135-136)
  const int nblk = xf_prep_blocks(Hr, Wr);
  DIM_RUN(launch_xf_gray(images_dev, channels, H, W, h->norm, h->partial, batch, Hr, Wr, s));
  DIM_RUN(launch_xf_stats(h->partial, nblk, Hr * Wr, h->stats, batch, s));
  DIM_RUN(launch_xf_normalize(h->norm, h->stats, batch, Hr * Wr, sat, s));
  // stem: block1 + skip1 (XFN:139-140)
  DIM_RUN(launch_xf_stem12(h->norm, h->stem, h->a2, batch, Hr, Wr, s));
  DIM_RUN(launch_xf_stem3(h->a2, h->stem, h->b2, batch, H2, W2, s));
  DIM_RUN(launch_xf_stem4(h->b2, h->norm, h->stem, h->q0, batch, H2, W2, sat, s));
  // trunk (XFN:140-143)
  DIM_RUN(conv(h->L[XF_L_BLOCK2], h->q0, H4, W4, h->q1, H4, W4, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK2 + 1], h->q1, H4, W4, h->q2, H4, W4, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK3], h->q2, H4, W4, h->e[0], H8, W8, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK3 + 1], h->e[0], H8, W8, h->e[1], H8, W8, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK3 + 2], h->e[1], H8, W8, h->e[2], H8, W8, false));      // x3
  DIM_RUN(conv(h->L[XF_L_BLOCK4], h->e[2], H8, W8, h->f[0], H16, W16, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK4 + 1], h->f[0], H16, W16, h->f[1], H16, W16, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK4 + 2], h->f[1], H16, W16, h->f[2], H16, W16, false));  // x4
  DIM_RUN(conv(h->L[XF_L_BLOCK5], h->f[2], H16, W16, h->g[0], H32, W32, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK5 + 1], h->g[0], H32, W32, h->g[1], H32, W32, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK5 + 2], h->g[1], H32, W32, h->g[2], H32, W32, false));
  DIM_RUN(conv(h->L[XF_L_BLOCK5 + 3], h->g[2], H32, W32, h->g3, H32, W32, false));    // x5
  // pyramid fusion (XFN:146-148): the sum is formed by a small kernel of its own (a 64-channel map at 1/8 resolution: 1.5 % of the stem's traffic),
  // not inside block_fusion.0's operand load, where every one of the nine taps would repeat the two bilinear blends
  DIM_RUN(launch_xf_fuse(h->e[2], h->f[2], h->g3, h->e[0], batch, H8, W8, sat, s));
  DIM_RUN(conv(h->L[XF_L_FUSION], h->e[0], H8, W8, h->e[1], H8, W8, false));
  DIM_RUN(conv(h->L[XF_L_FUSION + 1], h->e[1], H8, W8, h->e[0], H8, W8, false));
  DIM_RUN(conv(h->fusion2, h->e[0], H8, W8, h->e[3], H8, W8, false));                 // feats
  // reliability head (XFN:79-84) and the dense descriptors' normalisation (XFM:70)
  DIM_RUN(conv(h->L[XF_L_HEAT], h->e[3], H8, W8, h->e[0], H8, W8, false));
  DIM_RUN(conv(h->L[XF_L_HEAT + 1], h->e[0], H8, W8, h->e[1], H8, W8, false));
  DIM_RUN(launch_xf_dense_tail(h->e[1], h->heat_w, h->heat_b, h->e[3], h->h1, h->e[4], batch * H8 * W8, s));
  // keypoint head on the 8 x 8 unfolding of the normalised image (XFN:87-92,152), softmax + depth-to-space (XFM:242-247)
  DIM_RUN(conv(h->L[XF_L_KP], h->norm, Hr, Wr, h->e[0], H8, W8, true));
  DIM_RUN(conv(h->L[XF_L_KP + 1], h->e[0], H8, W8, h->e[1], H8, W8, false));
  DIM_RUN(conv(h->L[XF_L_KP + 2], h->e[1], H8, W8, h->e[0], H8, W8, false));
  DIM_RUN(launch_xf_kp_tail(h->e[0], h->kp_w, h->kp_b, h->k1h, batch, H8, W8, s));
  // selection (XFM:74-87) and the sparse tail (XFM:90-96)
  DIM_RUN(xf_select_chain(h->k1h, h->h1, h->key, h->cfg.detection_threshold, h->cfg.top_k, h->capacity, batch, Hr, Wr, h->rowcount, h->rowoff, h->ncand, h->cand_score,
                         h->cand_idx, h->topk_keys, h->kpts_px, scores_dev, (int*)n_kpts_dev, s));
  DIM_RUN(launch_xf_sparse(h->e[4], h->kpts_px, (const int*)n_kpts_dev, desc_dev, kpts_xy_dev, h->stride, h->capacity, batch, Hr, Wr, rw, rh, s));
  h->last_h = Hr; h->last_w = Wr;
  return 0;
}

int dim_xfeat_debug_buffers(dim_xfeat* h, const float** norm_image, const float** k1h, const float** h1, const float** m1, int* hr, int* wr) {
  DIM_REQUIRE(h, "dim_xfeat_debug_buffers: null handle");
  if (norm_image) *norm_image = h->norm;
  if (k1h) *k1h = h->k1h;
  if (h1) *h1 = h->h1;
  if (m1) *m1 = h->e[4];
  if (hr) *hr = h->last_h;
  if (wr) *wr = h->last_w;
  return 0;
}

size_t dim_op_xfeat_select_workspace_bytes(int batch, int H, int W, int top_k) {
  if (batch <= 0 || H <= 0 || W <= 0 || top_k <= 0) return 0;
  return xf_select_ws(batch, H, W, top_k).total;
}

int dim_op_xfeat_select(const float* k1h, const float* h1, int batch, int H, int W, float threshold, int top_k, int capacity, void* workspace, float* kpts_xy, float* scores,
                        int32_t* n_out, void* stream) {
  DIM_REQUIRE(k1h && h1 && workspace && kpts_xy && scores && n_out, "dim_op_xfeat_select: null argument");
  DIM_REQUIRE(batch > 0 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && (long long)batch * H * W <= 0x7fffffffLL, "dim_op_xfeat_select: bad map size %d x %d x %d", batch, H, W);
  DIM_REQUIRE(top_k > 0 && top_k <= capacity && capacity <= 32768, "dim_op_xfeat_select: top_k %d, capacity %d (top_k <= capacity <= 32768)", top_k, capacity);
  const XfSelectWs w = xf_select_ws(batch, H, W, top_k);
  char* base = (char*)workspace;
  unsigned long long* keys = topk_scratch_keys(batch, top_k) ? (unsigned long long*)(base + w.keys) : nullptr;
  return xf_select_chain(k1h, h1, (float*)(base + w.key), threshold, top_k, capacity, batch, H, W, (int*)(base + w.rowcount), (int*)(base + w.rowoff), (int*)(base + w.ncand),
                         (float*)(base + w.cand_score), (int*)(base + w.cand_idx), keys, kpts_xy, scores, (int*)n_out, (hipStream_t)stream);
}

}  // extern "C"
