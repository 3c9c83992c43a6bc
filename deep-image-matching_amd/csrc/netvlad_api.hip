// dim_netvlad_* : resident NetVLAD global-descriptor extractor (C ABI in include/dim_hip.h) and the operator entries of its two own kernels.
// Replaces thirdparty/hloc/extractors/netvlad.py (= NV) as hloc's extract_features.confs["netvlad"] drives it: VGG16 features[:-2] (NV:66-68),
// NetVLADLayer (NV:18-39), whitening (NV:143-144).
#include <string.h>

#include <vector>

#include "../../include/dim_hip.h"
#include "netvlad_kernels.h"

namespace {
constexpr int NV_NL = 13;
// torchvision's VGG16 "D" configuration without the last pool: cin, cout, pool after the layer's ReLU
struct NvGeo { int ci, co, pool; };
const NvGeo NV_VGG[NV_NL] = {{3, 64, 0}, {64, 64, 1}, {64, 128, 0}, {128, 128, 1}, {128, 256, 0}, {256, 256, 0}, {256, 256, 1},
                             {256, 512, 0}, {512, 512, 0}, {512, 512, 1}, {512, 512, 0}, {512, 512, 0}, {512, 512, 0}};
}  // namespace

struct dim_netvlad {
  DimHandleBase base;   // first member: dim_handle_tune_set
  int max_batch, max_h, max_w, K, whiten_out;
  float *mean, *w1, *bias[NV_NL];
  SplitWeights wsp[3][NV_NL];   // [mode 1 | 2][layer 1 ..]: bf16x6 and fp16x3 pieces
  float *score_dk, *centers_kd, *whiten_w, *whiten_b;
  float *act[2], *head_ws, *vlad, *whiten_ws;
  const float* last_map;   // conv5_3 map of the last call [last_batch][last_h][last_w][512]
  int last_batch, last_h, last_w;
};

extern "C" {

void dim_netvlad_destroy(dim_netvlad* h) {
  if (!h) return;
  dim_handle_release(&h->base);
  delete h;
}

int dim_netvlad_create(const dim_netvlad_weights* w, int max_batch, int max_h, int max_w, dim_netvlad** out) {
  DIM_REQUIRE(w && out, "dim_netvlad_create: null argument");
  DIM_REQUIRE(max_batch > 0 && max_batch <= 64, "dim_netvlad_create: max_batch %d outside [1, 64]", max_batch);
  DIM_REQUIRE(max_h >= 16 && max_w >= 16, "dim_netvlad_create: max_h %d / max_w %d below 16 (four pools)", max_h, max_w);
  // the 64-channel fp32 map of one image at full resolution must fit one buffer descriptor: what launch_conv3x3_x6_wide requires at extract time
  DIM_REQUIRE((long long)max_h * max_w * 64 * 4 < 0x7FFFFFF0LL, "dim_netvlad_create: %d x %d: the 64-channel map of one image exceeds 2 GiB (stay below 2^23 pixels)", max_h, max_w);
  const int K = w->K, WO = w->whiten_out;
  DIM_REQUIRE(K >= 8 && K <= NV_KMAX && K % 8 == 0, "dim_netvlad_create: %d clusters (a multiple of 8 up to %d)", K, NV_KMAX);
  for (int l = 0; l < NV_NL; ++l) {
    const NvGeo& g = NV_VGG[l];
    DIM_REQUIRE(w->conv_w[l] && w->conv_b[l], "dim_netvlad_create: convolution %d has a null tensor", l);
    DIM_REQUIRE(w->conv_w_elems[l] == (size_t)g.co * g.ci * 9, "dim_netvlad_create: conv_w[%d] has %zu elements, (%d, %d, 3, 3) expected", l, w->conv_w_elems[l], g.co, g.ci);
    DIM_REQUIRE(w->conv_b_elems[l] == (size_t)g.co, "dim_netvlad_create: conv_b[%d] has %zu elements, %d expected", l, w->conv_b_elems[l], g.co);
    DIM_REQUIRE(dim_all_finite(w->conv_w[l], w->conv_w_elems[l]) && dim_all_finite(w->conv_b[l], w->conv_b_elems[l]), "dim_netvlad_create: convolution %d holds a non-finite value", l);
  }
  DIM_REQUIRE(w->mean && w->mean_elems == 3, "dim_netvlad_create: mean has %zu elements, 3 expected", w->mean ? w->mean_elems : (size_t)0);
  DIM_REQUIRE(w->score_w && w->score_w_elems == (size_t)K * NV_D, "dim_netvlad_create: score_w has %zu elements, (%d, 512) expected", w->score_w ? w->score_w_elems : (size_t)0, K);
  DIM_REQUIRE(w->centers && w->centers_elems == (size_t)K * NV_D, "dim_netvlad_create: centers has %zu elements, (512, %d) expected", w->centers ? w->centers_elems : (size_t)0, K);
  DIM_REQUIRE(WO >= 0 && WO <= (1 << 20), "dim_netvlad_create: whiten_out %d", WO);
  if (WO > 0) {
    DIM_REQUIRE(w->whiten_w && w->whiten_w_elems == (size_t)WO * K * NV_D, "dim_netvlad_create: whiten_w has %zu elements, (%d, %d) expected", w->whiten_w ? w->whiten_w_elems : (size_t)0, WO, K * NV_D);
    DIM_REQUIRE(w->whiten_b && w->whiten_b_elems == (size_t)WO, "dim_netvlad_create: whiten_b has %zu elements, %d expected", w->whiten_b ? w->whiten_b_elems : (size_t)0, WO);
  } else {
    DIM_REQUIRE(!w->whiten_w && !w->whiten_b, "dim_netvlad_create: whitening tensors given with whiten_out 0");
  }
  std::unique_ptr<dim_netvlad, void (*)(dim_netvlad*)> guard(new dim_netvlad(), dim_netvlad_destroy);
  dim_netvlad* const h = guard.get();
  DimHandleBase* const hb = &h->base;
  h->max_batch = max_batch; h->max_h = max_h; h->max_w = max_w; h->K = K; h->whiten_out = WO;
  h->whiten_w = h->whiten_b = h->whiten_ws = nullptr;
  h->last_map = nullptr; h->last_batch = h->last_h = h->last_w = 0;

  DIM_TRY(dim_upload_f32(hb, &h->mean, w->mean, 3));
  {  // conv1_1: [(ci, dy, dx)][64]
    std::vector<float> k(27 * 64);
    for (int co = 0; co < 64; ++co)
      for (int j = 0; j < 27; ++j) k[(size_t)j * 64 + co] = w->conv_w[0][(size_t)co * 27 + j];
    DIM_TRY(dim_upload_f32(hb, &h->w1, k));
  }
  for (int l = 0; l < NV_NL; ++l) {
    const NvGeo& g = NV_VGG[l];
    DIM_TRY(dim_upload_f32(hb, &h->bias[l], w->conv_b[l], g.co));
    if (l == 0) continue;
    for (int mode = 1; mode <= 2; ++mode) {
      std::vector<unsigned short> hx(conv_split_weight_elems(g.ci, g.co, mode));
      SplitWeights& sw = h->wsp[mode][l];
      prepare_conv_weights_split(w->conv_w[l], g.ci, g.co, mode, hx.data(), &sw);
      DIM_TRY(dim_upload_split(hb, &sw, hx, mode, sw.n_pad));
    }
  }
  {  // head operands in kernel layout: scores (512, K), centres (K, 512)
    DIM_REQUIRE(dim_all_finite(w->score_w, w->score_w_elems) && dim_all_finite(w->centers, w->centers_elems), "dim_netvlad_create: the NetVLAD layer holds a non-finite value");
    std::vector<float> sdk((size_t)K * NV_D), ckd((size_t)K * NV_D);
    for (int k = 0; k < K; ++k)
      for (int d = 0; d < NV_D; ++d) {
        sdk[(size_t)d * K + k] = w->score_w[(size_t)k * NV_D + d];
        ckd[(size_t)k * NV_D + d] = w->centers[(size_t)d * K + k];
      }
    DIM_TRY(dim_upload_f32(hb, &h->score_dk, sdk));
    DIM_TRY(dim_upload_f32(hb, &h->centers_kd, ckd));
  }
  if (WO > 0) {
    DIM_TRY(dim_upload_f32(hb, &h->whiten_w, w->whiten_w, w->whiten_w_elems));
    DIM_TRY(dim_upload_f32(hb, &h->whiten_b, w->whiten_b, w->whiten_b_elems));
    DIM_TRY(dim_dev_alloc(hb, &h->whiten_ws, nv_whiten_workspace_floats(max_batch, K * NV_D, WO)));
  }
  const size_t B = max_batch, act = B * max_h * max_w * 64;   // the largest map: conv1_1 / conv1_2's 64 channels at full resolution
  DIM_TRY(dim_dev_alloc(hb, &h->act[0], act));
  DIM_TRY(dim_dev_alloc(hb, &h->act[1], act));
  DIM_TRY(dim_dev_alloc(hb, &h->head_ws, nv_head_workspace_floats(max_batch, (max_h / 16) * (max_w / 16), K)));
  DIM_TRY(dim_dev_alloc(hb, &h->vlad, B * K * NV_D));
  *out = guard.release();
  return 0;
}

int dim_netvlad_desc_dim(const dim_netvlad* h) { return h ? (h->whiten_out > 0 ? h->whiten_out : h->K * NV_D) : 0; }

int dim_netvlad_extract(dim_netvlad* h, const float* images_dev, int batch, int H, int W, float* desc_dev, void* stream) {
  DIM_REQUIRE(h && images_dev && desc_dev, "dim_netvlad_extract: null argument");
  DimTuneScope tune_scope(&h->base);
  DIM_REQUIRE(batch >= 1 && batch <= h->max_batch, "dim_netvlad_extract: batch %d outside [1,%d]", batch, h->max_batch);
  DIM_REQUIRE(H >= 16 && W >= 16 && H <= h->max_h && W <= h->max_w, "dim_netvlad_extract: image %dx%d outside [16x16, the handle's %dx%d]", H, W, h->max_h, h->max_w);
  hipStream_t s = (hipStream_t)stream;
  const int mode = dim_precision_mode() == 2 ? 2 : 1;   // fp16x3 under the range guard, else the bf16x6 split (no range limit)
  unsigned* const sat = mode == 2 ? dim_sat_counter(DIM_SAT_NETVLAD) : nullptr;
  float *cur = h->act[0], *nxt = h->act[1];
  int ch = H, cw = W;
  DIM_RUN(launch_nv_conv1(images_dev, h->mean, h->w1, h->bias[0], cur, batch, H, W, sat, s));
  for (int l = 1; l < NV_NL; ++l) {
    const NvGeo& g = NV_VGG[l];
    const int relu = l + 1 < NV_NL;   // features[:-2] ends on conv5_3 itself (NV:68)
    DIM_RUN(launch_conv3x3_x6_wide(cur, h->wsp[mode][l], h->bias[l], nxt, batch, ch, cw, g.ci, g.co, relu, s, sat));
    std::swap(cur, nxt);
    if (g.pool) {
      DIM_RUN(launch_nv_maxpool(cur, nxt, batch, ch, cw, g.co, s));
      std::swap(cur, nxt);
      ch /= 2; cw /= 2;
    }
  }
  h->last_map = cur; h->last_batch = batch; h->last_h = ch; h->last_w = cw;
  float* const vlad = h->whiten_out > 0 ? h->vlad : desc_dev;
  DIM_RUN(launch_nv_head(cur, batch, ch * cw, h->K, h->score_dk, h->centers_kd, h->head_ws, vlad, s));
  if (h->whiten_out > 0) DIM_RUN(launch_nv_whiten(vlad, batch, h->K * NV_D, h->whiten_w, h->whiten_b, h->whiten_out, h->whiten_ws, desc_dev, s));
  return 0;
}

int dim_netvlad_debug_buffers(dim_netvlad* h, const float** conv5_map, int* batch, int* mh, int* mw) {
  DIM_REQUIRE(h, "dim_netvlad_debug_buffers: null handle");
  if (conv5_map) *conv5_map = h->last_map;
  if (batch) *batch = h->last_batch;
  if (mh) *mh = h->last_h;
  if (mw) *mw = h->last_w;
  return 0;
}

size_t dim_op_netvlad_head_workspace_bytes(int batch, int n, int K) {
  if (batch <= 0 || n <= 0 || K <= 0) return 0;
  return nv_head_workspace_floats(batch, n, K) * sizeof(float);
}

int dim_op_netvlad_head_f32(const float* map_dev, int batch, int n, int K, const float* score_dk_dev, const float* centers_kd_dev, void* workspace,
                            float* vlad_dev, void* stream) {
  DIM_REQUIRE(map_dev && score_dk_dev && centers_kd_dev && workspace && vlad_dev, "dim_op_netvlad_head_f32: null argument");
  DIM_REQUIRE(batch >= 1, "dim_op_netvlad_head_f32: batch %d", batch);
  return launch_nv_head(map_dev, batch, n, K, score_dk_dev, centers_kd_dev, (float*)workspace, vlad_dev, (hipStream_t)stream);
}

size_t dim_op_netvlad_whiten_workspace_bytes(int batch, int in_dim, int out_dim) {
  if (batch <= 0 || in_dim <= 0 || out_dim <= 0) return 0;
  return nv_whiten_workspace_floats(batch, in_dim, out_dim) * sizeof(float);
}

int dim_op_netvlad_whiten_f32(const float* v_dev, int batch, int in_dim, const float* w_dev, const float* bias_dev, int out_dim, void* workspace,
                              float* y_dev, void* stream) {
  DIM_REQUIRE(v_dev && w_dev && bias_dev && workspace && y_dev, "dim_op_netvlad_whiten_f32: null argument");
  DIM_REQUIRE(batch >= 1, "dim_op_netvlad_whiten_f32: batch %d", batch);
  return launch_nv_whiten(v_dev, batch, in_dim, w_dev, bias_dev, out_dim, (float*)workspace, y_dev, (hipStream_t)stream);
}

}  // extern "C"
