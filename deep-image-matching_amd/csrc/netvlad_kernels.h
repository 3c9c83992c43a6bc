// Launchers of the NetVLAD global descriptor (netvlad.hip): the backbone's two small passes, the VLAD head and the whitening.
// thirdparty/hloc/extractors/netvlad.py = NV.  Everything runs on the caller's stream and never synchronises.
#pragma once
#include "dim_kernels.h"

constexpr int NV_D = 512;            // channels of the conv5_3 map
constexpr int NV_KMAX = 64;          // clusters: any multiple of 8 up to 64
constexpr int NV_WG_LOCS = 128;      // locations one workgroup of the head's first stage aggregates
constexpr int NV_WHITEN_KC = 4096;   // K range of one whitening workgroup (512 K is a multiple of it for every legal K)
constexpr int NV_WHITEN_NB = 16;     // images that share one pass over W

// conv1_1 with the input normalisation in its operand load (NV:126-130): image [b][H][W][3] in 0..1 -> clamp(255 x, 0, 255) - mean[c], zero padding
// AFTER the normalisation, 3 -> 64 channels, bias, ReLU; w [27 = (ci, dy, dx)][64], fp32 FMAs.  out [b][H][W][64].
int launch_nv_conv1(const float* image, const float* mean3, const float* w_27x64, const float* bias, float* out, int batch, int H, int W, unsigned* sat,
                    hipStream_t s);
// MaxPool2d(2, 2) with floor semantics (an odd last row / column is dropped): [b][H][W][C] -> [b][H / 2][W / 2][C], C % 4 == 0
int launch_nv_maxpool(const float* in, float* out, int batch, int H, int W, int C, hipStream_t s);

// The head on the conv5_3 map x [batch][n][512] (NV:138-139, NetVLADLayer.forward NV:28-39): vlad [batch][512 K], element d K + k.
// score_dk [512][K] (the checkpoint's own D x K layout), centers_kd [K][512] (NV:95 transposed).  workspace: nv_head_workspace_floats(batch, n, K) floats.
inline int nv_head_blocks(int n) { return (n + NV_WG_LOCS - 1) / NV_WG_LOCS; }
__host__ __device__ inline size_t nv_head_part_stride(int K) { return (size_t)K * NV_D + NV_KMAX; }
inline size_t nv_head_workspace_floats(int batch, int n, int K) { return (size_t)batch * nv_head_blocks(n) * nv_head_part_stride(K); }
int launch_nv_head(const float* x, int batch, int n, int K, const float* score_dk, const float* centers_kd, float* workspace, float* vlad, hipStream_t s);

// y = normalize(W v + b) (NV:143-144): v [batch][in_dim], W [out_dim][in_dim], y [batch][out_dim]; in_dim % NV_WHITEN_KC == 0.
// workspace: nv_whiten_workspace_floats(batch, in_dim, out_dim) floats.  W is read once per NV_WHITEN_NB images.
inline size_t nv_whiten_workspace_floats(int batch, int in_dim, int out_dim) {
  return (size_t)(in_dim / NV_WHITEN_KC) * (batch < NV_WHITEN_NB ? batch : NV_WHITEN_NB) * out_dim;
}
int launch_nv_whiten(const float* v, int batch, int in_dim, const float* W, const float* bias, int out_dim, float* workspace, float* y, hipStream_t s);
