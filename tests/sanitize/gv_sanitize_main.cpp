// Stand-alone sanitizer program (host code only, CPU): csrc/geom_verify.hip compiled against tests/hipemu, called at nk = 8193 (the
// streaming kernels, both chunk layouts) and nk = 100 (the LDS-resident kernels) from exactly sized heap blocks.  Built with
// -fsanitize=address,undefined and run by tests/test_geom_verify_sanitize.py; it needs nothing else of the library.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include <cmath>
#include "dim_hip.h"
// the two error-reporting entries geom_verify.hip takes from the rest of the library
static char g_err[1024];
void dim_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
extern "C" const char* dim_last_error(void) { return g_err; }

static int run(int nk, int n_pairs, const std::vector<int>& counts, const char* layout) {
  if (layout) setenv("DIM_GV_STREAM_LAYOUT", layout, 1); else unsetenv("DIM_GV_STREAM_LAYOUT");
  const int cap = nk;
  std::vector<float> kt((size_t)2 * n_pairs * cap * 2);
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / (float)(1u << 24); };
  // a planar-motion-free synthetic: x1 = x0 shifted by a depth-dependent disparity (a valid epipolar geometry), 30 % random
  for (int p = 0; p < n_pairs; ++p)
    for (int i = 0; i < cap; ++i) {
      const float x = rnd() * 1000.f, y = rnd() * 1000.f, d = 5.f + rnd() * 60.f;
      const bool out = rnd() < 0.3f;
      float* a = &kt[(((size_t)2 * p) * cap + i) * 2]; float* b = &kt[(((size_t)2 * p + 1) * cap + i) * 2];
      a[0] = x; a[1] = y; b[0] = out ? rnd() * 1000.f : x + d; b[1] = out ? rnd() * 1000.f : y + 0.1f * d;
    }
  // exactly sized heap blocks: any read or write past them is reported
  std::vector<int64_t> mt((size_t)n_pairs * nk * 2);
  for (int p = 0; p < n_pairs; ++p) for (int i = 0; i < nk; ++i) { mt[((size_t)p * nk + i) * 2] = i; mt[((size_t)p * nk + i) * 2 + 1] = (i * 7 + 3) % nk; }
  // (idx1 permuted: move image 1's keypoints accordingly)
  std::vector<float> k1((size_t)cap * 2);
  for (int p = 0; p < n_pairs; ++p) {
    float* b = &kt[(((size_t)2 * p + 1) * cap) * 2];
    for (int i = 0; i < nk; ++i) { const int j = (i * 7 + 3) % nk; k1[2 * j] = b[2 * i]; k1[2 * j + 1] = b[2 * i + 1]; }
    for (int i = 0; i < 2 * cap; ++i) b[i] = k1[i];
  }
  std::vector<int32_t> n(counts.begin(), counts.end());
  std::vector<unsigned char> scratch(dim_gv_scratch_bytes_nk(n_pairs, nk));
  std::vector<unsigned char> mask((size_t)n_pairs * nk);
  std::vector<int32_t> ninl(n_pairs);
  std::vector<double> F((size_t)n_pairs * 9);
  const int rc = dim_gv_fundamental(kt.data(), cap, nullptr, mt.data(), n.data(), nk, n_pairs, 2.0, 300, 0, 9u, scratch.data(), scratch.size(), mask.data(), ninl.data(), F.data(), nullptr);
  if (rc != 0) { printf("rc=%d %s\n", rc, dim_last_error()); return 1; }
  for (int p = 0; p < n_pairs; ++p) {
    int c = 0; for (int i = 0; i < nk; ++i) c += mask[(size_t)p * nk + i];
    printf("nk=%d layout=%s pair %d: n=%d inliers=%d mask.sum=%d\n", nk, layout ? layout : "default", p, n[p], ninl[p], c);
    if (c != ninl[p]) return 1;
  }
  return 0;
}
int main() {
  int bad = 0;
  bad |= run(8193, 3, {8193, 4097, 5}, nullptr);
  bad |= run(8193, 3, {8193, 4097, 5}, "double");
  bad |= run(100, 2, {100, 0}, nullptr);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
