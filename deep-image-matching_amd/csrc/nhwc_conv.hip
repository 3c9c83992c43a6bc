// The one implicit-GEMM NHWC convolution kernel of the small networks for gfx950 (ALIKE's encoder / aggregation layers, XFeat's trunk), its
// launcher, the host side of a layer (OIHW -> [K][N] operand, upload in both arithmetic forms) and the operator entry dim_op_nhwc_conv_f32.
// Arithmetic: fp16x3 on v_mfma_f32_32x32x16_f16 (SplitMma<2>, dim_common.h) by default, fp32 MFMA (v_mfma_f32_32x32x2_f32) otherwise.
// The accumulation order is fixed: tap-major, then 16-channel steps, then the in2 rows; no floating-point atomics.
#include "../../include/dim_hip.h"
#include "nhwc_conv.h"

namespace {

// ---------------------------------------------------------------------------
// Convolution as an implicit GEMM without LDS.  One wave owns an 8 wide x 4 tall tile of OUTPUT pixels (MFMA row i = pixel (i & 7, i >> 3)) and
// all NT 32-channel column tiles; a workgroup is 2 x 2 waves = 16 x 8 pixels.
// A operand (32x16 k-step): lane l supplies pixel i = l & 31, channels 16 c0 + 8 (l >> 5) + 0..7 of one tap: two 16-byte loads from
// the NHWC map, split on the fly.  B operand: split_weights' fragment order puts lane l's 8 halves of (plane, column tile, k-step)
// at 16-byte slot ((plane * NB + nt) * KS + ks) * 64 + l.
// C layout (dim_common.h): lane l, register r = row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 -> pixel x = (r & 3) + 4 (l >> 5),
// y = r >> 2: the 16 registers of a lane are one 4 x 4 pixel block of one channel, so both max-pools (alnet.py:101-102) reduce in registers.
// The operand forms (img3, unfold8, in2, stride) and the pooled epilogue are wave-uniform run-time branches on the argument struct.
template <int MODE, int NT>
__global__ __launch_bounds__(256) void nhwc_conv_kernel(const NhwcConv a, const unsigned short* __restrict__ wsplit, const float* __restrict__ inv_ch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.z;
  const int x0 = blockIdx.x * 16 + (wave & 1) * 8, y0 = blockIdx.y * 8 + (wave >> 1) * 4;
  const int i = lane & 31, kh = lane >> 5;
  const int px = x0 + (i & 7), py = y0 + (i >> 3);
  const bool p_ok = py < a.H && px < a.W;
  const int KS = (a.taps * a.cin_pad + a.cin2_pad) / 16;
  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

  auto step = [&](const float (&v)[8], int ks) {
    if constexpr (MODE == 2) {
      using P = SplitMma<2>;
      u32x4 ap[2];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned p[2];
        P::split(v[2 * e], v[2 * e + 1], P::act_scale(), p);
        ap[0][e] = p[0]; ap[1][e] = p[1];
      }
      const u32x4* wf = (const u32x4*)wsplit;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const u32x4 bh = wf[((size_t)(0 * NT + nt) * KS + ks) * 64 + lane], bl = wf[((size_t)(1 * NT + nt) * KS + ks) * 64 + lane];
        acc[nt] = P::mma(ap[1], bh, acc[nt]);   // smallest cross terms first: l*h, h*l, h*h
        acc[nt] = P::mma(ap[0], bl, acc[nt]);
        acc[nt] = P::mma(ap[0], bh, acc[nt]);
      }
    } else {
      // fp32 MFMA (32x32x2): call j contracts the channel pair {j, 8 + j} of the step: lane half kh supplies its own v[j] (channel 8 kh + j) and
      // the matching weight row, so no value changes lanes
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float* wrow = a.w32 + ((size_t)ks * 16 + 8 * kh + j) * a.n_pad + (lane & 31);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma32(v[j], wrow[nt * 32], acc[nt]);
      }
    }
  };
  // K runs over taps + 1 segments: the taps of `in` (cin_pad / 16 k-steps each), then the in2 rows.  A segment's k-step c is the lane's eight floats
  // at p + c * cstep, zeros when !ok.
  int ks = 0;
  for (int seg = 0; seg <= a.taps; ++seg) {
    const float* p;
    bool ok = p_ok;
    int n = a.cin_pad / 16, cstep = 16;
    if (seg == a.taps) {
      if (a.in2 == nullptr) break;
      n = a.cin2_pad / 16;
      p = a.in2 + (((size_t)b * a.H + (ok ? py : 0)) * a.W + (ok ? px : 0)) * a.cin2_pad + 8 * kh;
    } else if (a.unfold8) {
      // channel 16 c + 8 kh + j = row 2 c + kh, column j of the pixel's 8 x 8 block: eight consecutive floats of the plane
      cstep = 2 * a.in_w;
      p = a.in + ((size_t)b * a.in_h + 8 * (ok ? py : 0) + kh) * a.in_w + 8 * (ok ? px : 0);
    } else {
      const int dy = a.taps == 9 ? seg / 3 - 1 : 0, dx = a.taps == 9 ? seg % 3 - 1 : 0;
      const int yy = py * a.stride + dy, xx = px * a.stride + dx;
      ok = ok && yy >= 0 && yy < a.in_h && xx >= 0 && xx < a.in_w;
      const size_t pix = ((size_t)b * a.in_h + (ok ? yy : 0)) * a.in_w + (ok ? xx : 0);
      p = a.img3 ? a.in + pix * 3 : a.in + pix * a.cin_pad + 8 * kh;
      if (a.img3) ok = ok && kh == 0;   // one k-step per tap: channels 0..2 from lane half 0
    }
    for (int c = 0; c < n; ++c, p += cstep) {
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (ok) {
        if (a.img3) {
          v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
        } else {
          const float4 u0 = *(const float4*)p, u1 = *(const float4*)(p + 4);
          v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
        }
      }
      step(v, ks++);
    }
  }

  // epilogue: exact inverse scale of the split, folded BatchNorm / downsample bias, ReLU, store (+ pooled copy)
  float track = 0.f;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = nt * 32 + (lane & 31);
    const float inv = MODE == 2 ? inv_ch[col] : 1.0f, bias = a.bias[col];
    const bool col_ok = col < a.out_c;
    float val[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[nt][r] * inv + bias;
      if (a.relu) v = fmaxf(v, 0.f);
      val[r] = v;
      const int x = x0 + (r & 3) + 4 * kh, y = y0 + (r >> 2);
      if (col_ok && x < a.W && y < a.H) {
        a.out[(((size_t)b * a.H + y) * a.W + x) * a.out_c + col] = v;
        track = fmaxf(track, fabsf(v));
      }
    }
    if (a.pool == 4) {
      float m = val[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) m = fmaxf(m, val[r]);
      const int x = x0 + 4 * kh;
      if (col_ok && x < a.W && y0 < a.H) a.pooled[(((size_t)b * (a.H / 4) + y0 / 4) * (a.W / 4) + x / 4) * a.out_c + col] = m;
    } else if (a.pool == 2) {
#pragma unroll
      for (int qy = 0; qy < 2; ++qy)
#pragma unroll
        for (int qx = 0; qx < 2; ++qx) {
          const int r0 = (2 * qy) * 4 + 2 * qx;
          const float m = fmaxf(fmaxf(val[r0], val[r0 + 1]), fmaxf(val[r0 + 4], val[r0 + 5]));
          const int x = x0 + 4 * kh + 2 * qx, y = y0 + 2 * qy;
          if (col_ok && x < a.W && y < a.H) a.pooled[(((size_t)b * (a.H / 2) + y / 2) * (a.W / 2) + x / 2) * a.out_c + col] = m;
        }
    }
  }
  if (MODE == 2) sat_report(a.sat, track);
}

}  // namespace

int launch_nhwc_conv(const NhwcConv& a, bool x3, hipStream_t s) {
  DIM_REQUIRE(a.in && a.out && a.bias && a.w32 && (!x3 || (a.wx && a.wx->dev && a.wx->mode == 2 && a.wx->n_pad == a.n_pad)), "nhwc_conv: null operand");
  DIM_REQUIRE((a.taps == 9 || a.taps == 1) && a.cin_pad >= 16 && a.cin_pad % 16 == 0 && a.cin2_pad >= 0 && a.cin2_pad % 16 == 0 && a.out_c >= 16 && a.out_c % 16 == 0 &&
              a.n_pad % 32 == 0 && a.n_pad >= 32 && a.n_pad <= 128 && a.out_c <= a.n_pad, "nhwc_conv: channels (cin %d, cin2 %d, out %d, n_pad %d)", a.cin_pad,
              a.cin2_pad, a.out_c, a.n_pad);
  DIM_REQUIRE((a.in2 != nullptr) == (a.cin2_pad > 0), "nhwc_conv: in2 and cin2_pad %d go together", a.cin2_pad);
  DIM_REQUIRE(a.batch >= 1 && a.H >= 1 && a.W >= 1 && a.in_h >= 1 && a.in_w >= 1, "nhwc_conv: empty map");
  DIM_REQUIRE(a.stride == 1 || (a.stride == 2 && a.taps == 9), "nhwc_conv: stride %d with %d taps", a.stride, a.taps);
  DIM_REQUIRE(a.pool == 0 || ((a.pool == 2 || a.pool == 4) && a.pooled && a.H % a.pool == 0 && a.W % a.pool == 0), "nhwc_conv: pool %d on %dx%d", a.pool, a.H, a.W);
  // the combinations the networks use: stride and the unfolding come alone; the image layer has no in2
  DIM_REQUIRE(a.stride == 1 || (!a.img3 && !a.unfold8 && !a.in2 && a.pool == 0), "nhwc_conv: stride 2 with img3 / unfold8 / in2 / pool");
  DIM_REQUIRE(!a.unfold8 || (!a.img3 && !a.in2 && a.pool == 0), "nhwc_conv: unfold8 with img3 / in2 / pool");
  DIM_REQUIRE(!a.img3 || (a.cin_pad == 16 && !a.in2), "nhwc_conv: the image layer has one 16-channel k-step per tap and no in2");
  if (a.unfold8) DIM_REQUIRE(a.taps == 1 && a.cin_pad == 64 && a.in_h == 8 * a.H && a.in_w == 8 * a.W, "nhwc_conv: unfold of %dx%d into %dx%d", a.in_h, a.in_w, a.H, a.W);
  else if (!a.img3) DIM_REQUIRE((a.H - 1) * a.stride < a.in_h && (a.W - 1) * a.stride < a.in_w, "nhwc_conv: output %dx%d of input %dx%d at stride %d", a.H, a.W, a.in_h, a.in_w, a.stride);
  const dim3 grid(cdiv(a.W, 16), cdiv(a.H, 8), a.batch);
  const unsigned short* wsplit = x3 ? a.wx->dev : nullptr;
  const float* inv = x3 ? a.wx->inv_ch() : nullptr;
#define NHWC_CONV(MODE, NT) hipLaunchKernelGGL(HIP_KERNEL_NAME(nhwc_conv_kernel<MODE, NT>), grid, dim3(256), 0, s, a, wsplit, inv)
  switch ((x3 ? 10 : 0) + a.n_pad / 32) {
    case 1: NHWC_CONV(0, 1); break;
    case 2: NHWC_CONV(0, 2); break;
    case 3: NHWC_CONV(0, 3); break;
    case 4: NHWC_CONV(0, 4); break;
    case 11: NHWC_CONV(2, 1); break;
    case 12: NHWC_CONV(2, 2); break;
    case 13: NHWC_CONV(2, 3); break;
    default: NHWC_CONV(2, 4); break;
  }
#undef NHWC_CONV
  DIM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
void nhwc_conv_pack_oihw(std::vector<float>& kn, int N, int row0, const float* w, int co, int ci, int k, int cin_pad, const std::vector<double>* scale) {
  for (int a = 0; a < co; ++a)
    for (int b = 0; b < ci; ++b)
      for (int t = 0; t < k * k; ++t) {
        const float v = w[((size_t)a * ci + b) * k * k + t];
        kn[((size_t)row0 + (size_t)t * cin_pad + b) * N + a] = scale ? (float)((double)v * (*scale)[a]) : v;
      }
}

int nhwc_conv_upload(DimHandleBase* hb, NhwcConvLayer* L, const std::vector<float>& kn, int K, int N, const std::vector<float>& bias) {
  L->n_pad = dim_pad32(N); L->out_c = dim_pad16(N);
  DIM_TRY(dim_upload_gemm_split(hb, &L->wx, kn.data(), K, N, L->n_pad, 2));
  std::vector<float> w32((size_t)K * L->n_pad, 0.0f), b(L->n_pad, 0.0f);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) w32[(size_t)k * L->n_pad + n] = kn[(size_t)k * N + n];
  for (int n = 0; n < N; ++n) b[n] = bias[n];
  DIM_TRY(dim_upload_f32(hb, &L->w32, w32));
  DIM_TRY(dim_upload_f32(hb, &L->bias, b));
  return 0;
}

// ---------------------------------------------------------------------------
// operator entry (include/dim_hip.h): one layer as a handle, so that the kernel and the shared host code above are testable on their own
struct dim_nhwc_conv {
  DimHandleBase base;   // first member: owns the device memory
  NhwcConvLayer L;
};

extern "C" {

void dim_nhwc_conv_destroy(dim_nhwc_conv* h) {
  if (!h) return;
  dim_handle_release(&h->base);
  delete h;
}

int dim_nhwc_conv_create(const float* w_oihw, int cout, int cin, int ksize, int stride, const float* w2_oihw, int cin2, const float* bias, int relu, dim_nhwc_conv** out) {
  DIM_REQUIRE(w_oihw && bias && out, "dim_nhwc_conv_create: null argument");
  DIM_REQUIRE(cout >= 1 && cout <= 128 && cin >= 1 && (ksize == 3 || ksize == 1) && (stride == 1 || stride == 2) && cin2 >= 0 && (cin2 > 0) == (w2_oihw != nullptr),
              "dim_nhwc_conv_create: geometry (cout %d, cin %d, kernel %d, stride %d, cin2 %d)", cout, cin, ksize, stride, cin2);
  std::unique_ptr<dim_nhwc_conv, void (*)(dim_nhwc_conv*)> guard(new dim_nhwc_conv(), dim_nhwc_conv_destroy);
  NhwcConvLayer& L = guard->L;
  L.taps = ksize * ksize; L.stride = stride; L.relu = relu; L.cin_pad = dim_pad16(cin); L.cin2_pad = cin2 ? dim_pad16(cin2) : 0;
  const int K = L.taps * L.cin_pad + L.cin2_pad;
  std::vector<float> kn((size_t)K * cout, 0.0f);
  nhwc_conv_pack_oihw(kn, cout, 0, w_oihw, cout, cin, ksize, L.cin_pad, nullptr);
  if (cin2) nhwc_conv_pack_oihw(kn, cout, L.taps * L.cin_pad, w2_oihw, cout, cin2, 1, L.cin2_pad, nullptr);
  DIM_TRY(nhwc_conv_upload(&guard->base, &L, kn, K, cout, std::vector<float>(bias, bias + cout)));
  *out = guard.release();
  return 0;
}

int dim_op_nhwc_conv_f32(const dim_nhwc_conv* h, const float* in, int in_h, int in_w, int img3, int unfold8, const float* in2, float* out, float* pooled, int pool,
                         int batch, int H, int W, void* stream) {
  DIM_REQUIRE(h, "dim_op_nhwc_conv_f32: null handle");
  const NhwcConvLayer& L = h->L;
  DIM_REQUIRE((in2 != nullptr) == (L.cin2_pad > 0), "dim_op_nhwc_conv_f32: in2 must be given exactly when the layer was created with an in2 weight");
  NhwcConv a;
  a.in = in; a.cin_pad = L.cin_pad; a.taps = L.taps; a.stride = L.stride; a.in_h = in_h; a.in_w = in_w; a.img3 = img3 ? 1 : 0; a.unfold8 = unfold8 ? 1 : 0;
  a.in2 = in2; a.cin2_pad = L.cin2_pad;
  a.wx = &L.wx; a.w32 = L.w32; a.bias = L.bias; a.n_pad = L.n_pad; a.out = out; a.out_c = L.out_c; a.pooled = pooled; a.pool = pool; a.relu = L.relu;
  a.batch = batch; a.H = H; a.W = W; a.sat = dim_sat_counter(DIM_SAT_OP);
  return launch_nhwc_conv(a, dim_precision_mode() == 2, (hipStream_t)stream);
}

}  // extern "C"
