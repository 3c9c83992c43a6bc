// Launchers of the SuperGlue kernels (sg_kernels.hip): the keypoint encoder, the log-domain Sinkhorn passes and the match selection.  The graph
// network between them is a composition of the LightGlue launchers (sg_api.hip).  Everything is batched over pairs / items, ragged by
// n_cur[item], runs on the caller's stream and never synchronises.
#pragma once
#include "lg_kernels.h"

// Keypoint encoder weights (SGN:74-84), BatchNorm already folded into the convolutions by the host: [in][out] operands
struct SgEncW {
  const float* w[5];   // [3][32], [32][64], [64][128], [128][256], [256][256]
  const float* b[5];
};
// Optimal-transport state of a handle: u [pairs][nmax + 1], v [pairs][nmax + 1] (pair p of m x n keypoints: u[0..m) rows, u[m] the dustbin row;
// v[0..n), v[n] the dustbin column), the selection's scratch and the bin score.
struct SgOt {
  float* u; float* v;
  int* arg0; int* arg1;     // [pairs][nmax] row / column argmax over the real block
  float* val0;              // [pairs][nmax] the row maximum of Z + u + v - norm
  float alpha;
};

// st.n_cur / st.done from the tables (an empty side: done = -1, every later launch skips the pair), k' = (k - size / 2) / (0.7 max(W, H)) with
// size_tab rows (W, H), the five-stage MLP over [x', y', score], desc = desc_tab + MLP.  `sat`: fp16x3 range guard on the stored descriptors.
int launch_sg_encoder(const LgState& st, const SgEncW& w, const float* kpts_tab, const float* desc_tab, const float* score_tab, const int* n_tab,
                      const float* size_tab, const int* pair_idx, int cap, unsigned* sat, hipStream_t s);
// one Sinkhorn half-iteration for every pair of the call (SGN:152-186 on the coupling matrix that is never built: st.sim holds the m x n block,
// the dustbin row / column / corner are the scalar alpha).  rows: u = log_mu - LSE_j(Z + v); cols: v = log_nu - LSE_i(Z + u).
int launch_sg_sinkhorn_rows(const LgState& st, const SgOt& ot, hipStream_t s);
int launch_sg_sinkhorn_cols(const LgState& st, const SgOt& ot, hipStream_t s);
// row / column argmax of Z + u + v - norm over the real block (lowest index wins), mutual check, exp(max) > thr (SGN:288-305); outputs in the
// layout of dim_lg_match (out_cap = row stride of the per-point arrays)
int launch_sg_select(const LgState& st, const SgOt& ot, float thr, int out_cap, long long* matches, float* mscores, int* n_matches, int* mfull,
                     float* msfull, hipStream_t s);
