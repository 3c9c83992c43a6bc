// C-ABI: error reporting + operator-level entry points (thin wrappers over the
// internal launchers so each kernel can be parity-tested on its own).
#include <stdarg.h>
#include <stdio.h>

#include "../../include/dim_hip.h"
#include "lg_kernels.h"
#include "sp_kernels.h"

static thread_local char g_err[1024] = "";

void dim_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#include <vector>
namespace {
unsigned long long g_prof_mask = 0ull;
std::vector<hipEvent_t> g_prof_ev;  // begin/end pairs
size_t g_prof_used = 0;
}  // namespace

// ---- fp16x3 range guard: one block of sticky counters per device, allocated on first use ----
namespace {
constexpr int kMaxDev = 16;
unsigned* g_sat_dev[kMaxDev] = {nullptr};
bool g_sat_failed[kMaxDev] = {false};
unsigned g_sat_host[DIM_SAT_SITES] = {0};
__global__ void read_clocks_kernel(unsigned long long* out) {
  out[0] = (unsigned long long)__builtin_readcyclecounter();
  out[1] = (unsigned long long)wall_clock64();
}
unsigned* sat_block() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDev) return nullptr;
  if (!g_sat_dev[d] && !g_sat_failed[d]) {
    void* p = nullptr;
    if (hipMalloc(&p, DIM_SAT_SITES * sizeof(unsigned)) != hipSuccess || hipMemset(p, 0, DIM_SAT_SITES * sizeof(unsigned)) != hipSuccess) g_sat_failed[d] = true;
    else g_sat_dev[d] = (unsigned*)p;
  }
  return g_sat_dev[d];
}
}  // namespace
unsigned* dim_sat_counter(int site) {
  unsigned* b = sat_block();
  return (b && site >= 0 && site < DIM_SAT_SITES) ? b + site : nullptr;
}
void dim_sat_host_bump(int site) {
  if (site >= 0 && site < DIM_SAT_SITES) g_sat_host[site]++;
}

// process defaults (dim_tune_set) with per-handle overrides (dim_handle_tune_set): see DimTuneScope in dim_common.h
static thread_local const DimTune* g_tune_scope = nullptr;
void dim_tune_scope_set(const DimTune* t) { g_tune_scope = t; }
const DimTune* dim_tune_scope_get() { return g_tune_scope; }
// the device memory of a handle (DimHandleBase in dim_common.h)
int dim_dev_alloc_bytes(DimHandleBase* b, void** p, size_t bytes) {
  void* q = nullptr;
  const hipError_t e = hipMalloc(&q, bytes + DIM_ALLOC_SLACK);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    dim_set_error("hipMalloc of %zu bytes failed: out of memory (%s)", bytes, hipGetErrorString(e));
    return -1;
  }
  b->allocs.push_back(q);
  b->bytes += bytes;
  *p = q;
  return 0;
}
int dim_upload_bytes(DimHandleBase* b, void** dst, const void* src, size_t bytes) {
  if (dim_dev_alloc_bytes(b, dst, bytes) != 0) return -1;
  if (hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    dim_set_error("weight upload failed");
    return -1;
  }
  return 0;
}
int dim_upload_f32(DimHandleBase* b, float** dst, const float* src, size_t count) {
  if (!dim_all_finite(src, count)) { dim_set_error("non-finite value in the weights"); return -1; }
  return dim_upload(b, dst, src, count);
}
int dim_upload_split(DimHandleBase* b, SplitWeights* sw, const std::vector<unsigned short>& host, int mode, int n_pad) {
  unsigned short* d = nullptr;
  if (dim_upload(b, &d, host.data(), host.size()) != 0) return -1;
  sw->dev = d; sw->mode = mode; sw->n_pad = n_pad;
  return 0;
}
int dim_upload_gemm_split(DimHandleBase* b, SplitWeights* sw, const float* w_kn, int K, int N, int n_pad, int mode, int kperm) {
  if (!dim_all_finite(w_kn, (size_t)K * N)) { dim_set_error("non-finite value in the weights"); return -1; }
  std::vector<unsigned short> host(gemm_split_weight_elems(K, n_pad, mode));
  split_weights(w_kn, K, N, n_pad, mode, host.data(), sw, kperm);
  return dim_upload_split(b, sw, host, mode, n_pad);
}
void dim_handle_release(DimHandleBase* b) {
  for (void* p : b->allocs) hipFree(p);
  b->allocs.clear();
  b->bytes = 0;
}
static inline int tuned(int key, int process_default) {
  const DimTune* t = g_tune_scope;
  return (t && t->v[key] >= 0) ? t->v[key] : process_default;
}
static int g_precision_mode = 2;
int dim_precision_mode() { return tuned(1, g_precision_mode); }
static int g_fuse_conv1a = 1;
int dim_fuse_conv1a() { return tuned(3, g_fuse_conv1a); }
static int g_fuse_sp_head = 1;
int dim_fuse_sp_head() { return tuned(16, g_fuse_sp_head); }
static int g_fold_out_proj = 1;
int dim_fold_out_proj() { return tuned(4, g_fold_out_proj); }
static int g_fuse_kv = 1;
int dim_fuse_kv() { return tuned(8, g_fuse_kv); }
static int g_follow_stop = 1;
int dim_follow_stop_flags() { return tuned(18, g_follow_stop); }
static int g_defer_assign = 1;
int dim_defer_assignment() { return tuned(17, g_defer_assign); }
static int g_fuse_ffn_ln = 3;
int dim_fuse_ffn_ln() { return tuned(11, g_fuse_ffn_ln); }
#ifdef DIM_RESEARCH   // research build (build.build_variant("research")): prototype / timing-probe selectors, see dim_kernels.h
static int g_gemm_kc = 32;
int dim_gemm_kc() { return g_gemm_kc; }
static int g_conv_wino = 0;
int dim_conv_winograd() { return g_conv_wino; }
static int g_gemm_probe = 0;
int dim_gemm_probe() { return g_gemm_probe; }
static int g_attn_probe = 0;
int dim_attn_probe() { return g_attn_probe; }
#endif
#ifdef DIM_RESEARCH   // the research build keeps the dense descriptor head
int dim_sparse_desc() { return 0; }
#else
static int g_sparse_desc = 1;
int dim_sparse_desc() { return tuned(20, g_sparse_desc); }
#endif
static int g_al_tile_rows = 16;
int dim_aliked_tile_rows() { return tuned(10, g_al_tile_rows); }
static int g_al_fuse_bn = 1;
int dim_aliked_fuse_bn() { return tuned(9, g_al_fuse_bn); }
static int g_presplit = 1;
int dim_presplit_activations() { return tuned(5, g_presplit); }

void dim_prof_begin(int site, hipStream_t s) {
  if (!((g_prof_mask >> site) & 1ull)) return;
  if (g_prof_used + 2 > g_prof_ev.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    g_prof_ev.push_back(a); g_prof_ev.push_back(b);
  }
  hipEventRecord(g_prof_ev[g_prof_used], s);
}
void dim_prof_end(int site, hipStream_t s) {
  if (!((g_prof_mask >> site) & 1ull) || g_prof_used + 2 > g_prof_ev.size()) return;
  hipEventRecord(g_prof_ev[g_prof_used + 1], s);
  g_prof_used += 2;
}

extern "C" {

int dim_profile_start(unsigned long long site_mask) {
  g_prof_mask = site_mask;
  g_prof_used = 0;
  return 0;
}

int dim_profile_stop(double* total_ms, int* launches) {
  DIM_REQUIRE(total_ms && launches, "dim_profile_stop: null argument");
  double tot = 0.0;
  for (size_t i = 0; i + 1 < g_prof_used; i += 2) {
    DIM_HIP(hipEventSynchronize(g_prof_ev[i + 1]));
    float ms = 0.f;
    DIM_HIP(hipEventElapsedTime(&ms, g_prof_ev[i], g_prof_ev[i + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *launches = (int)(g_prof_used / 2);
  g_prof_mask = 0ull;
  g_prof_used = 0;
  return 0;
}

int dim_saturation_read(unsigned* counts_host, unsigned long long* total, int reset, void* stream) {
  unsigned c[DIM_SAT_SITES] = {0};
  unsigned* b = sat_block();
  if (b) {
    DIM_HIP(hipMemcpyAsync(c, b, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (reset) DIM_HIP(hipMemsetAsync(b, 0, sizeof(c), (hipStream_t)stream));
    DIM_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
  unsigned long long tot = 0;
  for (int i = 0; i < DIM_SAT_SITES; ++i) {
    c[i] += g_sat_host[i];
    if (reset) g_sat_host[i] = 0;
    tot += c[i];
    if (counts_host) counts_host[i] = c[i];
  }
  if (total) *total = tot;
  return 0;
}

int dim_saturation_reset(void* stream) {
  unsigned* b = sat_block();
  if (b) DIM_HIP(hipMemsetAsync(b, 0, DIM_SAT_SITES * sizeof(unsigned), (hipStream_t)stream));
  for (int i = 0; i < DIM_SAT_SITES; ++i) g_sat_host[i] = 0;
  return 0;
}

int dim_op_read_clocks(unsigned long long* out_dev, void* stream) {
  DIM_REQUIRE(out_dev, "dim_op_read_clocks: null argument");
  hipLaunchKernelGGL(read_clocks_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, out_dev);
  DIM_LAUNCH_CHECK();
  return 0;
}

const char* dim_last_error(void) { return g_err; }

int dim_abi_version(void) { return DIM_HIP_ABI_VERSION; }

int dim_op_gemm_f32(const float* A, int lda, const float* B, int ldb, int b_is_nk, const float* bias,
                    const float* residual, int ldr, float* C, int ldc, int M, int N, int K, int relu, void* stream) {
  GemmArgs g;
  g.A0 = A; g.lda0 = lda; g.B = B; g.ldb = ldb; g.bt = b_is_nk; g.bias = bias;
  g.R = residual; g.ldr = ldr; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.relu = relu;
  return launch_gemm(g, 1, (hipStream_t)stream);
}

int dim_op_conv3x3_nhwc_f32(const float* in, const float* w_tap_cin_cout, const float* bias, float* out, int batch,
                            int H, int W, int cin, int cout, int pool2x2, int relu, void* stream) {
  return launch_conv3x3(in, w_tap_cin_cout, bias, out, batch, H, W, cin, cout, pool2x2, relu, (hipStream_t)stream);
}

int dim_op_conv1a_f32(const float* in, const float* w_tap_cout, const float* bias, float* out, int batch, int H,
                      int W, void* stream) {
  return launch_conv1a(in, w_tap_cout, bias, out, batch, H, W, (hipStream_t)stream);
}

int dim_op_simple_nms_f32(const float* score_map, float* out, int batch, int H, int W, int radius, void* stream) {
  return launch_nms(score_map, out, batch, H, W, radius, (hipStream_t)stream);
}

// Keypoint selection as the extractors run it (sp_api.hip / aliked_api.hip): launch_select_ex -> launch_topk [-> launch_topk_zero_fill], on tables
// carved out of the caller's workspace (256-byte aligned pieces; nothing is allocated here).
namespace {
struct SelectTopkWs {
  size_t rowcount, rowoff, ncand, cand_score, cand_idx, keys, total;   // byte offsets
};
SelectTopkWs select_topk_ws(int batch, int H, int W, int k) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t rows = (size_t)batch * H, px = rows * W;
  SelectTopkWs w;
  w.rowcount = 0;
  w.rowoff = w.rowcount + up(rows * 4);
  w.ncand = w.rowoff + up(rows * 4);
  w.cand_score = w.ncand + up((size_t)batch * 4);
  w.cand_idx = w.cand_score + up(px * 4);
  w.keys = w.cand_idx + up(px * 4);
  w.total = w.keys + up(topk_scratch_keys(batch, k) * 8);
  return w;
}
}  // namespace

size_t dim_op_select_topk_workspace_bytes(int batch, int H, int W, int k) {
  if (batch <= 0 || H <= 0 || W <= 0) return 0;
  return select_topk_ws(batch, H, W, k).total;
}

int dim_op_select_topk_f32(const float* nms, int batch, int H, int W, float threshold, const float* threshold_dev, int border, int k,
                           int capacity, int sort_always, int zero_fill, void* workspace, float* kpts_xy, float* scores, int32_t* n_out,
                           int32_t* n_candidates, void* stream) {
  DIM_REQUIRE(nms && workspace && kpts_xy && scores && n_out, "dim_op_select_topk_f32: null argument");
  DIM_REQUIRE(batch > 0 && H > 0 && W > 0 && (long long)batch * H * W <= 0x7fffffffLL, "dim_op_select_topk_f32: bad map size %d x %d x %d", batch, H, W);
  DIM_REQUIRE(capacity > 0 && k != 0 && border >= 0, "dim_op_select_topk_f32: capacity %d must be > 0, k %d non-zero (negative: keep all), border %d >= 0", capacity, k, border);
  DIM_REQUIRE(k <= capacity, "dim_op_select_topk_f32: k %d > capacity %d", k, capacity);
  DIM_REQUIRE(!(zero_fill && threshold_dev), "dim_op_select_topk_f32: zero_fill takes the scalar threshold only");
  if (zero_fill) DIM_REQUIRE((long long)k <= (long long)H * W, "selected index k out of range: top_k %d > %d x %d pixels", k, H, W);   // launch_topk_zero_fill's check, before anything runs
  const SelectTopkWs w = select_topk_ws(batch, H, W, k);
  char* base = (char*)workspace;
  int* ncand = n_candidates ? (int*)n_candidates : (int*)(base + w.ncand);
  unsigned long long* keys = topk_scratch_keys(batch, k) ? (unsigned long long*)(base + w.keys) : nullptr;
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_select_ex(nms, batch, H, W, threshold, threshold_dev, border, (int*)(base + w.rowcount), (int*)(base + w.rowoff), ncand,
                            (float*)(base + w.cand_score), (int*)(base + w.cand_idx), 0, s);
  if (rc != 0) return rc;
  rc = launch_topk((const float*)(base + w.cand_score), (const int*)(base + w.cand_idx), ncand, batch, H, W, k, capacity, kpts_xy, scores, (int*)n_out,
                   keys, sort_always ? 1 : 0, s);
  if (rc != 0) return rc;
  if (zero_fill) rc = launch_topk_zero_fill(nms, batch, H, W, threshold, border, k, capacity, kpts_xy, scores, (int*)n_out, s);
  return rc;
}

int dim_op_sample_descriptors_f32(const float* dense_nhwc, const float* kpts_xy, const int32_t* n_kpts, float* desc, int batch, int h, int w,
                                  int capacity, int fix_sampling, void* stream) {
  DIM_REQUIRE(dense_nhwc && kpts_xy && n_kpts && desc, "dim_op_sample_descriptors_f32: null argument");
  DIM_REQUIRE(batch > 0 && h > 0 && w > 0 && capacity > 0, "dim_op_sample_descriptors_f32: bad size (batch %d, %d x %d cells, capacity %d)", batch, h, w, capacity);
  return launch_sample_desc(dense_nhwc, kpts_xy, (const int*)n_kpts, desc, batch, h, w, capacity, fix_sampling, (hipStream_t)stream);
}

// Op-level handles: a host struct holding the pre-split device operand for the precision mode that was active
// at creation (dim_tune_set key 1: 2 = fp16x3, 1 = bf16x6).
static int x3_create(const float* w_kn_host, int K, int N, void** out_dev, int* n_pad_out, int kperm);
int dim_x3_create(const float* w_kn_host, int K, int N, void** out_dev, int* n_pad_out) { return x3_create(w_kn_host, K, N, out_dev, n_pad_out, 0); }
int dim_x3_create_kperm(const float* w_kn_host, int K, int N, void** out_dev, int* n_pad_out) { return x3_create(w_kn_host, K, N, out_dev, n_pad_out, 1); }
static int x3_create(const float* w_kn_host, int K, int N, void** out_dev, int* n_pad_out, int kperm) {
  DIM_REQUIRE(w_kn_host && out_dev && n_pad_out && K > 0 && N > 0, "dim_x3_create: bad argument");
  const int mode = g_precision_mode == 1 ? 1 : 2;
  const int n_pad = (N + 127) / 128 * 128;
  std::vector<unsigned short> host(gemm_split_weight_elems(K, n_pad, mode));
  SplitWeights* w = new SplitWeights();
  split_weights(w_kn_host, K, N, n_pad, mode, host.data(), w, kperm);
  void* d = nullptr;
  if (hipMalloc(&d, host.size() * 2) != hipSuccess || hipMemcpy(d, host.data(), host.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
    delete w;
    dim_set_error("dim_x3_create: device allocation / upload failed (out of memory?)");
    return -1;
  }
  w->dev = (const unsigned short*)d; w->mode = mode; w->n_pad = n_pad;
  *out_dev = w; *n_pad_out = n_pad;
  return 0;
}
void dim_x3_destroy(void* handle) {
  if (!handle) return;
  SplitWeights* w = (SplitWeights*)handle;
  hipFree((void*)w->dev);
  delete w;
}
int dim_op_gemm_x6_f32(const float* A, int lda, const void* w_x3, int n_pad, const float* bias, const float* residual, int ldr,
                       float* C, int ldc, int M, int N, int K, int act, void* stream) {
  DIM_REQUIRE(w_x3 && ((const SplitWeights*)w_x3)->n_pad == n_pad, "dim_op_gemm_x6_f32: bad weight handle");
  GemmArgs g;
  g.A0 = A; g.lda0 = lda; g.set_split(*(const SplitWeights*)w_x3); g.bias = bias;
  g.R = residual; g.ldr = ldr; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.relu = act;
  g.sat = dim_sat_counter(DIM_SAT_OP);
  return launch_gemm_x6(g, 1, (hipStream_t)stream);
}

int dim_op_gemm_x6_ln_gelu_f32(const float* A, int lda, const void* w_x3, const float* bias, const float* ln_gamma, const float* ln_beta,
                               float* C, int ldc, int M, int K, void* stream) {
  DIM_REQUIRE(w_x3 && ((const SplitWeights*)w_x3)->n_pad == 512 && ((const SplitWeights*)w_x3)->mode == 2, "dim_op_gemm_x6_ln_gelu_f32: needs an fp16x3 512-column weight handle");
  DIM_REQUIRE(A && bias && ln_gamma && ln_beta && C, "dim_op_gemm_x6_ln_gelu_f32: null argument");
  GemmArgs g;
  g.A0 = A; g.lda0 = lda; g.set_split(*(const SplitWeights*)w_x3); g.bias = bias; g.ln_gamma = ln_gamma; g.ln_beta = ln_beta;
  g.C = C; g.ldc = ldc; g.M = M; g.N = 512; g.K = K;
  g.sat = dim_sat_counter(DIM_SAT_OP);
  return launch_gemm_x6(g, 1, (hipStream_t)stream);
}

int dim_op_gemm_x6_nt_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, void* stream) {
  DIM_REQUIRE(A && B && C && g_precision_mode != 0, "dim_op_gemm_x6_nt_f32: null argument, or the fp32 arithmetic is selected");
  GemmArgs g;
  g.A0 = A; g.lda0 = lda; g.B = B; g.ldb = ldb; g.bt = 1; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  return launch_gemm_x6_nt(g, 1, g_precision_mode == 1 ? 1 : 2, (hipStream_t)stream);
}

int dim_op_ffn_fused_f32(const float* A, int lda, const void* w0_x3, const float* bias0, const float* ln_gamma, const float* ln_beta,
                         const void* w3_x3_kperm, const float* bias3, const float* residual, int ldr, float* C, int ldc, int M, int K, void* stream) {
  DIM_REQUIRE(w0_x3 && ((const SplitWeights*)w0_x3)->n_pad == 512 && ((const SplitWeights*)w0_x3)->mode == 2, "dim_op_ffn_fused_f32: needs an fp16x3 512-column ffn.0 handle");
  DIM_REQUIRE(w3_x3_kperm && ((const SplitWeights*)w3_x3_kperm)->n_pad == 256 && ((const SplitWeights*)w3_x3_kperm)->mode == 2, "dim_op_ffn_fused_f32: needs an fp16x3 256-column ffn.3 handle (dim_x3_create_kperm)");
  DIM_REQUIRE(A && bias0 && ln_gamma && ln_beta && bias3 && residual && C, "dim_op_ffn_fused_f32: null argument");
  GemmArgs g;
  g.A0 = A; g.lda0 = lda; g.set_split(*(const SplitWeights*)w0_x3); g.bias = bias0; g.ln_gamma = ln_gamma; g.ln_beta = ln_beta;
  g.set_split2(*(const SplitWeights*)w3_x3_kperm); g.bias2 = bias3; g.R = residual; g.ldr = ldr;
  g.C = C; g.ldc = ldc; g.M = M; g.N = 512; g.K = K;
  g.sat = dim_sat_counter(DIM_SAT_OP); g.sat2 = dim_sat_counter(DIM_SAT_OP);
  return launch_gemm_x6(g, 1, (hipStream_t)stream);
}

// LightGlue / LighterGlue / SuperGlue attention as the matchers run it (lg_api.hip, lgl_api.hip, sg_api.hip): an LgState over the caller's tensors, the K | V
// tile images and the key-split partial records carved out of the caller's workspace (256-byte aligned pieces; nothing is allocated here), then the
// matchers' own launchers.
namespace {
struct LgAttentionWs {
  size_t kv_img, part, total;   // byte offsets
};
LgAttentionWs lg_attention_ws(int width, int n_items, int nmax, int split_items) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t tiles = (size_t)cdiv(nmax, 32);
  LgAttentionWs w;
  w.kv_img = 0;
  // [items][4 heads][tiles][KV_TILE_STRIDE x 16 B] (lg_attn_x6.hip) / [items][tiles][2304 x 16 B] (lg_attn_d96.hip)
  w.part = up(width == 256 ? (size_t)n_items * 4 * tiles * KV_TILE_STRIDE * 16 : (size_t)n_items * tiles * 2304 * 16);
  // [split_items][4 heads][nmax][4 parts][68] / [split_items][nmax][4 parts][100] floats
  w.total = w.part + up(split_items > 0 ? (size_t)split_items * nmax * 4 * (width == 256 ? 4 * 68 : 100) * sizeof(float) : 0);
  return w;
}
int lg_attention_state(LgState& st, const char* who, int width, int kind, float* qkv, const float* enc, const int32_t* n_dev, const int32_t* done_dev,
                       float* ctx, int n_items, int nmax, int nsel, int split_items, void* workspace) {
  DIM_REQUIRE(width == 256 || width == 96, "%s: width %d (256: four heads of 64; 96: one head)", who, width);
  DIM_REQUIRE(kind >= 0 && kind <= (width == 256 ? 3 : 1), "%s: kind %d at width %d (0 self, 1 cross; 2 / 3 SuperGlue self / cross at width 256)", who, kind, width);
  DIM_REQUIRE(qkv && n_dev && done_dev && ctx && workspace, "%s: null argument", who);
  DIM_REQUIRE(enc || kind != 0, "%s: self attention (kind 0) needs the rotary table", who);
  DIM_REQUIRE(n_items >= 2 && n_items % 2 == 0, "%s: n_items %d must be a positive even number (item = 2 * pair + side)", who, n_items);
  DIM_REQUIRE(nmax > 0 && nsel > 0 && nsel <= nmax && split_items >= 0, "%s: need 0 < nsel %d <= nmax %d and split_items %d >= 0", who, nsel, nmax, split_items);
  DIM_REQUIRE((long long)n_items * nmax * 3 * width <= 0x7fffffffLL, "%s: %d items of %d rows exceed 2^31 elements", who, n_items, nmax);
  const LgAttentionWs w = lg_attention_ws(width, n_items, nmax, split_items);
  char* base = (char*)workspace;
  st.n_pairs = n_items / 2; st.n_items = n_items; st.nmax = nmax; st.nsel = nsel;
  st.qkv = qkv; st.ctx = ctx; st.enc = (float*)enc; st.n_cur = (int*)n_dev; st.done = (int*)done_dev;
  st.kv_img = base + w.kv_img;
  st.attn_part = split_items > 0 ? (float*)(base + w.part) : nullptr;
  st.attn_part_items = split_items;
  st.sat_qkv = dim_sat_counter(DIM_SAT_OP);
  st.sg = kind >= 2 ? 1 : 0;
  if (width == 96) { st.dim = 96; st.heads = 1; st.head_dim = 96; }
  return 0;
}
}  // namespace

size_t dim_op_lg_attention_workspace_bytes(int width, int n_items, int nmax, int split_items) {
  if ((width != 256 && width != 96) || n_items <= 0 || nmax <= 0 || split_items < 0) return 0;
  return lg_attention_ws(width, n_items, nmax, split_items).total;
}

int dim_op_lg_attention_f32(int width, int kind, float* qkv, const float* enc, const int32_t* n_dev, const int32_t* done_dev, float* ctx, int n_items,
                            int nmax, int nsel, int split_items, void* workspace, void* stream) {
  LgState st{};
  int rc = lg_attention_state(st, "dim_op_lg_attention_f32", width, kind, qkv, enc, n_dev, done_dev, ctx, n_items, nmax, nsel, split_items, workspace);
  if (rc != 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int mode = dim_precision_mode();
  if (width == 96) return launch_lgl_attention(st, kind, s);   // (refuses the fp32 arithmetic itself)
  if (kind >= 2) {   // as dim_sg_match
    DIM_REQUIRE(mode == 1 || mode == 2, "dim_op_lg_attention_f32: SuperGlue attention exists in the split arithmetics (fp16x3, bf16x6) only, not fp32");
    return launch_lg_attention_x6(st, kind & 1, s, 0);
  }
  if (mode == 0 && kind == 0) {   // the split kernels rotate q and k while they load them; the fp32 kernel reads them rotated (dim_lg_match)
    rc = launch_lg_rotary(st, s);
    if (rc != 0) return rc;
  }
  return launch_lg_attention(st, kind, s, 0);
}

int dim_op_lg_qkv_attention_f32(int kind, const float* x, const void* w_x3, const float* bias, const float* enc, const int32_t* n_dev,
                                const int32_t* done_dev, float* qkv, float* ctx, int n_items, int nmax, int nsel, int split_items, void* workspace,
                                void* stream) {
  const char* who = "dim_op_lg_qkv_attention_f32";
  DIM_REQUIRE(kind == 0 || kind == 1, "%s: kind %d (0 self, 1 cross)", who, kind);
  DIM_REQUIRE(x && w_x3 && bias, "%s: null argument", who);
  const SplitWeights& W = *(const SplitWeights*)w_x3;
  const int N = kind == 0 ? 768 : 512;
  DIM_REQUIRE(dim_precision_mode() == 2 && W.mode == 2 && W.n_pad == N, "%s: needs the fp16x3 arithmetic and an fp16x3 weight handle of 256 x %d (dim_x3_create)", who, N);
  LgState st{};
  int rc = lg_attention_state(st, who, 256, kind, qkv, enc, n_dev, done_dev, ctx, n_items, nmax, nsel, split_items, workspace);
  if (rc != 0) return rc;
  DIM_REQUIRE(gemm_x6_fuses_kv(nsel, N, n_items, 2), "%s: the projection GEMM does not write K | V tile images at %d items of %d rows x %d columns "
              "(gemm_x6_fuses_kv is false: neither the 128 x 256 nor the 32 x 128 block runs this shape)", who, n_items, nsel, N);
  hipStream_t s = (hipStream_t)stream;
  GemmArgs g;   // lg_api.hip gemm_qkv
  g.A0 = x; g.lda0 = 256; g.strideA0 = (long long)nmax * 256;
  g.bias = bias; g.C = qkv; g.ldc = 768; g.strideC = (long long)nmax * 768;
  g.M = nsel; g.N = N; g.K = 256; g.rows = st.n_cur; g.flag = st.done; g.flag_shift = 1; g.flag_eq = 0;
  g.sat = st.sat_qkv;
  g.kv_img = st.kv_img; g.kv_tiles = cdiv(nmax, 32); g.kv_kblock = kind == 0 ? 1 : 0; g.kv_vblock = g.kv_kblock + 1; g.kv_nmax = nmax;
  g.kv_enc = kind == 0 ? enc : nullptr;
  g.set_split(W);
  rc = launch_gemm_x6(g, n_items, s);
  if (rc != 0) return rc;
  return launch_lg_attention(st, kind, s, 1);
}

// LightGlue / LighterGlue confidence, decision, pruning, assignment and finalize as the matchers run them (lg_api.hip, lgl_api.hip): an LgState over the
// caller's tensors, then the matchers' own launchers.  `need` names the pointers the entry uses; the others stay as the caller gave them.
namespace {
enum : unsigned {
  HS_DESC = 1u << 0, HS_ENC = 1u << 1, HS_SIM = 1u << 2, HS_CONF = 1u << 3, HS_MTCH = 1u << 4, HS_ZLS = 1u << 5, HS_RMAX = 1u << 6, HS_RLSE = 1u << 7,
  HS_BEST = 1u << 8, HS_ARG = 1u << 9, HS_NCUR = 1u << 10, HS_NNEW = 1u << 11, HS_NORIG = 1u << 12, HS_IND = 1u << 13, HS_DEST = 1u << 14,
  HS_PRUNE = 1u << 15, HS_DONE = 1u << 16, HS_CNT = 1u << 17
};
int lg_head_state(LgState& st, const char* who, const dim_lg_head_state* hs, unsigned need) {
  DIM_REQUIRE(hs != nullptr, "%s: null state", who);
  DIM_REQUIRE(hs->width == 256 || hs->width == 96, "%s: width %d (256: LightGlue; 96: LighterGlue)", who, hs->width);
  DIM_REQUIRE(hs->n_pairs > 0 && hs->nmax > 0 && hs->nsel > 0 && hs->nsel <= hs->nmax, "%s: need n_pairs %d > 0 and 0 < nsel %d <= nmax %d", who,
              hs->n_pairs, hs->nsel, hs->nmax);
  DIM_REQUIRE((long long)hs->n_pairs * 2 * hs->nmax * 256 <= 0x7fffffffLL, "%s: %d pairs of %d rows exceed 2^31 elements", who, hs->n_pairs, hs->nmax);
  const void* ptr[18] = {hs->desc, hs->enc, hs->sim, hs->conf, hs->mtch, hs->zls, hs->rmax, hs->rlse, hs->best, hs->arg, hs->n_cur, hs->n_new,
                         hs->n_orig, hs->ind, hs->dest, hs->prune, hs->done, hs->cnt_lt};
  static const char* const name[18] = {"desc", "enc", "sim", "conf", "mtch", "zls", "rmax", "rlse", "best", "arg", "n_cur", "n_new",
                                       "n_orig", "ind", "dest", "prune", "done", "cnt_lt"};
  for (int i = 0; i < 18; ++i) DIM_REQUIRE(!((need >> i) & 1u) || ptr[i] != nullptr, "%s: null %s", who, name[i]);
  st.n_pairs = hs->n_pairs; st.n_items = 2 * hs->n_pairs; st.nmax = hs->nmax; st.nsel = hs->nsel;
  st.desc = hs->desc; st.enc = hs->enc; st.sim = hs->sim; st.conf = hs->conf; st.mtch = hs->mtch; st.zls = hs->zls; st.rmax = hs->rmax;
  st.rlse = hs->rlse; st.best = hs->best; st.arg = (int*)hs->arg; st.n_cur = (int*)hs->n_cur; st.n_new = (int*)hs->n_new; st.n_orig = (int*)hs->n_orig;
  st.ind = (int*)hs->ind; st.dest = (int*)hs->dest; st.prune = (int*)hs->prune; st.done = (int*)hs->done; st.cnt_lt = (int*)hs->cnt_lt;
  if (hs->width == 96) { st.dim = 96; st.heads = 1; st.head_dim = 96; }
  return 0;
}
struct LgPruneWs {
  size_t tdesc, tenc, tind, total;   // byte offsets
};
LgPruneWs lg_prune_ws(int width, int n_items, int nmax) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t rows = (size_t)n_items * nmax;
  LgPruneWs w;
  w.tdesc = 0;
  w.tenc = w.tdesc + up(rows * width * sizeof(float));
  w.tind = w.tenc + up(rows * (width == 256 ? 64 : 96) * sizeof(float));
  w.total = w.tind + up(rows * sizeof(int));
  return w;
}
}  // namespace

int dim_op_lg_confidence_f32(const dim_lg_head_state* hs, const float* w_tok, const float* b_tok, const float* w_match, const float* b_match, float thr,
                             int use_token, void* stream) {
  const char* who = "dim_op_lg_confidence_f32";
  LgState st{};
  int rc = lg_head_state(st, who, hs, HS_DESC | HS_CONF | HS_MTCH | HS_CNT | HS_NCUR | HS_DONE);
  if (rc != 0) return rc;
  DIM_REQUIRE(w_match && b_match && (!use_token || (w_tok && b_tok)), "%s: null weights", who);
  if (hs->width == 96) return launch_lgl_confidence(st, w_tok, b_tok, w_match, b_match, thr, use_token ? 1 : 0, (hipStream_t)stream);
  return launch_lg_confidence(st, w_tok, b_tok, w_match, b_match, thr, use_token ? 1 : 0, (hipStream_t)stream);
}

int dim_op_lg_decide(const dim_lg_head_state* hs, int layer, float depth_conf, int early, int last, void* stream) {
  const char* who = "dim_op_lg_decide";
  LgState st{};
  int rc = lg_head_state(st, who, hs, HS_DONE | HS_CNT | HS_NORIG);
  if (rc != 0) return rc;
  DIM_REQUIRE(layer >= 0, "%s: layer %d", who, layer);
  return launch_lg_decide(st, layer, depth_conf, early ? 1 : 0, last ? 1 : 0, (hipStream_t)stream, nullptr);
}

size_t dim_op_lg_prune_workspace_bytes(int width, int n_items, int nmax) {
  if ((width != 256 && width != 96) || n_items <= 0 || nmax <= 0) return 0;
  return lg_prune_ws(width, n_items, nmax).total;
}

int dim_op_lg_prune(const dim_lg_head_state* hs, int layer, double width_conf, float thr, int use_token, int pruning_min, void* workspace, void* stream) {
  const char* who = "dim_op_lg_prune";
  LgState st{};
  int rc = lg_head_state(st, who, hs, HS_DESC | HS_ENC | HS_CONF | HS_MTCH | HS_NCUR | HS_NNEW | HS_IND | HS_DEST | HS_PRUNE | HS_DONE);
  if (rc != 0) return rc;
  DIM_REQUIRE(workspace && layer >= 0, "%s: null workspace, or layer %d", who, layer);
  const LgPruneWs w = lg_prune_ws(hs->width, st.n_items, st.nmax);
  char* base = (char*)workspace;
  st.tdesc = (float*)(base + w.tdesc); st.tenc = (float*)(base + w.tenc); st.tind = (int*)(base + w.tind);
  return launch_lg_prune(st, layer, width_conf, thr, use_token ? 1 : 0, pruning_min, (hipStream_t)stream);
}

int dim_op_lg_assign_f32(const dim_lg_head_state* hs, int tag, const float* w_match, const float* b_match, float* dense, void* stream) {
  const char* who = "dim_op_lg_assign_f32";
  LgState st{};
  int rc = lg_head_state(st, who, hs, HS_DESC | HS_SIM | HS_ZLS | HS_RMAX | HS_RLSE | HS_BEST | HS_ARG | HS_NCUR | HS_DONE);
  if (rc != 0) return rc;
  DIM_REQUIRE(w_match && b_match && tag >= 0, "%s: null weights, or tag %d < 0", who, tag);
  rc = launch_lg_assign_stats(st, tag, w_match, b_match, (hipStream_t)stream);
  if (rc != 0) return rc;
  return launch_lg_assign_argmax(st, tag, dense, (hipStream_t)stream);
}

int dim_op_lg_finalize(const dim_lg_head_state* hs, int n_layers, int prune_enabled, float filter_thr, int out_cap, int64_t* matches, float* mscores,
                       int32_t* n_matches, int32_t* mfull, float* msfull, int32_t* stop, int32_t* prune_out, void* stream) {
  const char* who = "dim_op_lg_finalize";
  LgState st{};
  int rc = lg_head_state(st, who, hs, HS_BEST | HS_ARG | HS_NCUR | HS_NORIG | HS_IND | HS_DONE | (prune_enabled ? HS_PRUNE : 0u));
  if (rc != 0) return rc;
  DIM_REQUIRE(matches && mscores && n_matches && mfull && msfull && stop && prune_out && out_cap > 0, "%s: null output, or out_cap %d", who, out_cap);
  return launch_lg_finalize(st, n_layers, prune_enabled ? 1 : 0, filter_thr, out_cap, (long long*)matches, mscores, (int*)n_matches, (int*)mfull, msfull,
                            (int*)stop, (int*)prune_out, (hipStream_t)stream);
}

int dim_convx6_create(const float* w_oihw_host, int cin, int cout, void** out_dev) {
  DIM_REQUIRE(w_oihw_host && out_dev && (cin == 64 || cin == 128) && cout % 64 == 0, "dim_convx6_create: bad argument");
  const int mode = g_precision_mode == 1 ? 1 : 2;
  std::vector<unsigned short> host(conv_split_weight_elems(cin, cout, mode));
  SplitWeights* w = new SplitWeights();
  prepare_conv_weights_split(w_oihw_host, cin, cout, mode, host.data(), w);
  void* d = nullptr;
  if (hipMalloc(&d, host.size() * 2) != hipSuccess || hipMemcpy(d, host.data(), host.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
    delete w;
    dim_set_error("dim_convx6_create: device allocation / upload failed (out of memory?)");
    return -1;
  }
  w->dev = (const unsigned short*)d; w->mode = mode;
  *out_dev = w;
  return 0;
}
int dim_op_conv3x3_x6_nhwc_f32(const float* in, const void* w_x6, const float* bias, float* out, int batch, int H, int W,
                               int cin, int cout, int pool2x2, int relu, void* stream) {
  DIM_REQUIRE(w_x6, "dim_op_conv3x3_x6_nhwc_f32: null weight handle");
  return launch_conv3x3_x6(in, *(const SplitWeights*)w_x6, bias, out, batch, H, W, cin, cout, pool2x2, relu, (hipStream_t)stream, dim_sat_counter(DIM_SAT_OP));
}

int dim_tune_set(int key, int value) {
  if (key == 0) dim_conv_set_variant(value);
  if (key == 1) g_precision_mode = value;
  if (key == 2) dim_conv_x6_set_variant(value);
  if (key == 3) g_fuse_conv1a = value;
  if (key == 4) g_fold_out_proj = value;
  if (key == 5) g_presplit = value;
  if (key == 6) dim_gemm_x6_set_wide(value);
  if (key == 7) dim_nms_set_big_tiles(value);
  if (key == 8) g_fuse_kv = value;
  if (key == 9) g_al_fuse_bn = value;
  if (key == 10) g_al_tile_rows = value;
  if (key == 11) g_fuse_ffn_ln = value;
  if (key == 16) g_fuse_sp_head = value;
  if (key == 17) g_defer_assign = value;
  if (key == 18) g_follow_stop = value;
#ifndef DIM_RESEARCH
  if (key == 20) g_sparse_desc = value;
#endif
#ifdef DIM_RESEARCH
  if (key == 12) g_attn_probe = value;
  if (key == 13) g_gemm_probe = value;
  if (key == 14) g_gemm_kc = value;
  if (key == 15) g_conv_wino = value;
#else
  DIM_REQUIRE(key < 12 || key > 15, "dim_tune_set: key %d selects a research prototype / timing probe that the product library does not contain "
              "(build.build_variant(\"research\", [\"-DDIM_RESEARCH\"]) -> libdim_hip_research.so)", key);
#endif
  DIM_REQUIRE((key >= 0 && key <= 18) || key == 20, "dim_tune_set: unknown key %d", key);
  return 0;
}

int dim_handle_tune_set(void* handle, int key, int value) {
  DimHandleBase* b = (DimHandleBase*)handle;
  DIM_REQUIRE(b != nullptr && b->magic == DIM_HANDLE_MAGIC, "dim_handle_tune_set: not an extractor / matcher handle of this library");
  DIM_REQUIRE(key == 1 || key == 3 || key == 4 || key == 5 || key == 8 || key == 9 || key == 10 || key == 11 || key == 16 || key == 17 || key == 18 || key == 20,
              "dim_handle_tune_set: key %d has no per-handle form (arithmetic 1; fusion 3, 4, 5, 8, 9, 11, 16, 17, 18, 20; ALIKED tile rows 10)", key);
  b->tune.v[key] = value < 0 ? -1 : value;
  return 0;
}

int dim_device_synchronize(void) {
  DIM_HIP(hipDeviceSynchronize());
  return 0;
}

}  // extern "C"
