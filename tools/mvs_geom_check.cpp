// A host program around diner::mvs_taps (diner_amd/csrc/mvs_geom.hpp), the one place where the matching stage's similarity kernels turn
// a homography and a depth hypothesis into addresses -- addresses the backward pass scatters to.  Built for the host alone, with
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan tools/mvs_geom_check.cpp
// (tests/test_match_grad_cpu.py does that), it feeds the function adversarial depths and homography entries -- NaN, +-inf, +-1e30, the
// largest float, denormals, zeros, values that put the sample exactly on -1, 0, size - 1 and size -- at every pixel of small maps (1 x 1
// and 1 x N among them) and at the corners of large ones, and checks that
//   * every index lies in [0, H W), whatever the inputs are;
//   * every weight is finite and lies in [0, 1];
//   * an invalid sample (z component below 1e-6, or NaN coordinates) carries four zero weights;
//   * a tap outside the map carries a zero weight, and for a finite sample inside the map the indices name the pixels floor() names.
// Prints the number of samples checked and exits 0, or prints the first violation and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../diner_amd/csrc/mvs_geom.hpp"

namespace {

long long g_checked = 0;

[[noreturn]] void fail(const char* what, const float* hm, int x, int y, float z, int H, int W) {
  std::printf("FAIL: %s at x %d y %d z %.9g of %d x %d, hom", what, x, y, (double)z, H, W);
  for (int i = 0; i < 12; ++i) std::printf(" %.9g", (double)hm[i]);
  std::printf("\n");
  std::exit(1);
}

void check(const float* hm, int x, int y, float z, int H, int W) {
  const diner::MvsTaps t = diner::mvs_taps(hm, x, y, z, H, W);
  ++g_checked;
  for (int i = 0; i < 4; ++i) {
    if (t.idx[i] < 0 || t.idx[i] >= H * W) fail("an index is out of range", hm, x, y, z, H, W);
    if (!std::isfinite(t.wt[i])) fail("a weight is not finite", hm, x, y, z, H, W);
    if (!(t.wt[i] >= 0.0f && t.wt[i] <= 1.0f)) fail("a weight is outside [0, 1]", hm, x, y, z, H, W);
  }
  // the rule, restated: the projected point in fp32 as the kernel forms it
  const float fx = (float)x, fy = (float)y;
  const float rx = fmaf(hm[1], fy, hm[0] * fx) + hm[2], ry = fmaf(hm[4], fy, hm[3] * fx) + hm[5], rz = fmaf(hm[7], fy, hm[6] * fx) + hm[8];
  const float px3 = fmaf(rx, z, hm[9]), py3 = fmaf(ry, z, hm[10]), pz3 = fmaf(rz, z, hm[11]);
  const float qx = px3 / pz3, qy = py3 / pz3;
  const bool invalid = pz3 < 1e-6f;
  if (invalid || std::isnan(qx) || std::isnan(qy)) {
    for (int i = 0; i < 4; ++i)
      if (t.wt[i] != 0.0f) fail("an invalid sample carries a weight", hm, x, y, z, H, W);
    return;
  }
  const bool outside = !(qx > -1.0f && qx < (float)W && qy > -1.0f && qy < (float)H);
  if (outside) {
    for (int i = 0; i < 4; ++i)
      if (t.wt[i] != 0.0f) fail("a sample outside the map carries a weight", hm, x, y, z, H, W);
    return;
  }
  const long long x0 = (long long)std::floor((double)qx), y0 = (long long)std::floor((double)qy);
  for (int i = 0; i < 4; ++i) {
    const long long xi = x0 + (i & 1), yi = y0 + (i >> 1);
    const bool in = xi >= 0 && xi < W && yi >= 0 && yi < H;
    if (!in && t.wt[i] != 0.0f) fail("a tap outside the map carries a weight", hm, x, y, z, H, W);
    if (in && (long long)t.idx[i] != yi * W + xi) fail("a tap inside the map names another pixel", hm, x, y, z, H, W);
  }
  const float tx = qx - (float)x0, ty = qy - (float)y0;
  const float want[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
  for (int i = 0; i < 4; ++i) {
    const long long xi = x0 + (i & 1), yi = y0 + (i >> 1);
    if (xi >= 0 && xi < W && yi >= 0 && yi < H && t.wt[i] != want[i]) fail("a weight differs from the fp32 product", hm, x, y, z, H, W);
  }
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float big = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
  const std::vector<float> bad = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1e-6f, 9.9e-7f, 1e30f, -1e30f, big, -big, inf, -inf, nan, tiny, -tiny,
                                  1e-38f, 2147483648.0f, -2147483648.0f, 4294967296.0f, 1e10f, -1e10f, 16777216.0f};
  const int sizes[][2] = {{1, 1}, {1, 7}, {5, 1}, {1, 640}, {4, 5}, {23, 37}, {512, 640}, {3, 46340}, {46340, 3}, {16384, 16384}};
  const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  for (const auto& hw : sizes) {
    const int H = hw[0], W = hw[1];
    std::vector<int> ys = {0, H / 2, H - 1}, xs = {0, W / 2, W - 1};
    if (H <= 40 && W <= 60) {
      ys.clear();
      xs.clear();
      for (int y = 0; y < H; ++y) ys.push_back(y);
      for (int x = 0; x < W; ++x) xs.push_back(x);
    }
    for (int y : ys)
      for (int x : xs) {
        // depths: with rot = identity and a translation, (x z + tx) / z; every bad value as the depth
        for (float z : bad) check(identity, x, y, z, H, W);
        // every entry of the homography replaced by every bad value, at a plain and at a bad depth
        for (int e = 0; e < 12; ++e)
          for (float v : bad) {
            float hm[12];
            for (int i = 0; i < 12; ++i) hm[i] = identity[i];
            hm[e] = v;
            for (float z : {1.0f, 1.5f, nan, inf, -1e30f, tiny}) check(hm, x, y, z, H, W);
          }
        // translations that put the sample exactly on -1, 0, size - 1, size and one ulp to either side (depth 1: the sample is x + t)
        for (float target : {-2.0f, -1.0f, 0.0f, (float)(W - 1), (float)W, (float)W + 1.0f, (float)W + 2.0f})
          for (float t : {target - (float)x, std::nextafterf(target - (float)x, inf), std::nextafterf(target - (float)x, -inf)}) {
            float hm[12];
            for (int i = 0; i < 12; ++i) hm[i] = identity[i];
            hm[9] = t;
            check(hm, x, y, 1.0f, H, W);
            hm[10] = t;
            check(hm, x, y, 1.0f, H, W);
          }
        for (float target : {-2.0f, -1.0f, 0.0f, (float)(H - 1), (float)H, (float)H + 1.0f, (float)H + 2.0f})
          for (float t : {target - (float)y, std::nextafterf(target - (float)y, inf), std::nextafterf(target - (float)y, -inf)}) {
            float hm[12];
            for (int i = 0; i < 12; ++i) hm[i] = identity[i];
            hm[10] = t;
            check(hm, x, y, 1.0f, H, W);
          }
      }
  }
  std::printf("mvs_geom_check: %lld samples, every index in range\n", g_checked);
  return 0;
}
