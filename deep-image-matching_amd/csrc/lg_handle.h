// The resident matcher handle behind the dim_lg_* C ABI, shared by its two creators: dim_lg_create (lg_api.hip, LightGlue: width 256, four heads
// of 64) and dim_lgl_create (lgl_api.hip, LighterGlue: width 96, one head of 96).
#pragma once
#include <vector>

#include "../../include/dim_hip.h"
#include "lg_kernels.h"

struct LayerW {
  float *qkv_w, *qkv_b, *out_w, *out_b, *sffn0_w, *sffn0_b, *sln_w, *sln_b, *sffn3_w, *sffn3_b;
  float *cqkv_w, *cqkv_b, *cout_w, *cout_b, *cffn0_w, *cffn0_b, *cln_w, *cln_b, *cffn3_w, *cffn3_b;
  float *match_w, *match_b, *proj_w, *proj_b, *tok_w, *tok_b;
  // pre-split copies of the GEMM operands for the split modes 1 (bf16x6) and 2 (fp16x3), gemm_x6.hip; index = mode
  SplitWeights qkv_x[3], out_x[3], sffn0_x[3], sffn3_x[3], cqkv_x[3], cout_x[3], cffn0_x[3], cffn3_x[3], proj_x[3];
  // out_proj folded into ffn.0 (split modes): [desc | ctx] * [W1a ; Wout*W1b] + (b1 + bout*W1b)
  SplitWeights sffn0f_x[3], cffn0f_x[3];
  SplitWeights sffn3p_x[3], cffn3p_x[3];   // ffn.3 with the k permutation of the fused feed-forward kernel (gemm_x6.hip, KV == 4)
  float *sffn0f_b, *cffn0f_b;
};

struct dim_lg {
  DimHandleBase base;   // first member: dim_handle_tune_set
  dim_lg_config cfg;
  int n_layers, input_dim, max_pairs, nmax;
  std::vector<LayerW> L;
  std::vector<float> thr;
  float *inproj_w, *inproj_b, *Wr;
  // the deferred assignment of adaptive depth (dim_lg_match): per-layer tables the kernels index with a pair's stop layer
  float *match_w_all = nullptr, *match_b_all = nullptr;   // [layers][256], [layers]
  GemmLayerTab* proj_tab[3] = {nullptr, nullptr, nullptr};   // [mode][layers]: final_proj's split weights / inverse scales / bias
  // adaptive depth at one or two pairs per call: the host follows the stop flags two layers behind the device (dim_lg_match)
  int* done_host = nullptr;            // page-locked, device-mapped: [layers][max_pairs flags | sequence word] written by lg_decide_kernel
  int call_seq = 0;
  LgState st;   // st.dim / heads / head_dim: 256 / 4 / 64 (dim_lg_create) or 96 / 1 / 96 (dim_lgl_create, lgl_api.hip)
};

// dim_lg_match on a handle of width 96 (lgl_api.hip); arguments already validated by dim_lg_match
int lgl_match(dim_lg* h, const float* kpts_tab_dev, const float* desc_tab_dev, const int32_t* n_tab_dev, const float* size_tab_dev, int cap,
              const int32_t* pair_idx_dev, int n_pairs, int64_t* matches_dev, float* mscores_dev, int32_t* n_matches_dev, int32_t* matches01_dev,
              float* mscores01_dev, int32_t* stop_dev, int32_t* prune01_dev, float* dense_scores_dev, hipStream_t s);
