// A host program around diner::deform_corners (diner_amd/csrc/deform_geom.hpp), the one place where the deformable convolution turns
// learned offsets into addresses.  Built for the host alone, with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/deform_geom_check.cpp
// (tests/test_featurenet_cpu.py does that), it feeds the function adversarial offsets -- huge, infinite, NaN, exactly -1, exactly
// H - 1, exactly H, one ulp to either side of each -- at every pixel and tap of several map sizes and checks that
//   * every index marked valid lies in [0, H W) and is the pixel (y, x) the float64 statement of the rule names;
//   * a sample the rule calls outside marks nothing valid and carries four zero weights;
//   * the weights are finite, in [0, 1], and equal the fp32 products hy hx, hy lx, ly hx, ly lx;
//   * a corner is marked valid exactly when it lies inside the image.
// Prints the number of samples checked and exits 0, or prints the first violation and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../diner_amd/csrc/deform_geom.hpp"

namespace {

long long g_checked = 0;

[[noreturn]] void fail(const char* what, int h, int w, int ky, int kx, float dy, float dx, int H, int W) {
  std::printf("FAIL: %s at h %d w %d tap (%d,%d) dy %.9g dx %.9g of %d x %d\n", what, h, w, ky, kx, (double)dy, (double)dx, H, W);
  std::exit(1);
}

void check(int h, int w, int ky, int kx, float dy, float dx, int H, int W) {
  const diner::DeformCorners c = diner::deform_corners(h, w, ky, kx, dy, dx, H, W);
  ++g_checked;
  // the rule in float64 on the fp32 coordinate (the coordinate itself is one fp32 addition by definition)
  const float pyf = (float)(h - 1 + ky) + dy, pxf = (float)(w - 1 + kx) + dx;
  const double py = pyf, px = pxf;
  const bool outside = std::isnan(py) || std::isnan(px) || py <= -1.0 || py >= (double)H || px <= -1.0 || px >= (double)W;
  if (outside) {
    if (c.valid != 0u) fail("an outside sample marks a corner valid", h, w, ky, kx, dy, dx, H, W);
    for (int i = 0; i < 4; ++i)
      if (c.wt[i] != 0.0f || c.idx[i] != 0) fail("an outside sample carries a weight or an index", h, w, ky, kx, dy, dx, H, W);
    return;
  }
  const double y0 = std::floor(py), x0 = std::floor(px);
  const float ly = pyf - (float)y0, lx = pxf - (float)x0, hy = 1.0f - ly, hx = 1.0f - lx;
  const float want_wt[4] = {hy * hx, hy * lx, ly * hx, ly * lx};
  for (int i = 0; i < 4; ++i) {
    const long long y = (long long)y0 + (i >> 1), x = (long long)x0 + (i & 1);
    const bool in = y >= 0 && y <= H - 1 && x >= 0 && x <= W - 1;
    const bool marked = (c.valid >> i) & 1u;
    if (marked != in) fail("a corner's validity differs from the rule", h, w, ky, kx, dy, dx, H, W);
    if (marked) {
      if (c.idx[i] < 0 || c.idx[i] >= H * W) fail("a valid index is out of range", h, w, ky, kx, dy, dx, H, W);
      if ((long long)c.idx[i] != y * W + x) fail("a valid index names another pixel", h, w, ky, kx, dy, dx, H, W);
    } else if (c.idx[i] != 0) {
      fail("an invalid corner carries an index", h, w, ky, kx, dy, dx, H, W);
    }
    if (!(c.wt[i] >= 0.0f && c.wt[i] <= 1.0f)) fail("a weight is outside [0, 1]", h, w, ky, kx, dy, dx, H, W);
    if (c.wt[i] != want_wt[i]) fail("a weight differs from the fp32 product", h, w, ky, kx, dy, dx, H, W);
  }
  if (c.valid & ~15u) fail("bits beyond the four corners", h, w, ky, kx, dy, dx, H, W);
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float big = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
  const int sizes[][2] = {{1, 1}, {1, 7}, {5, 1}, {4, 5}, {9, 19}, {36, 52}, {512, 640}, {3, 46340}, {46340, 3}, {16384, 16384}};
  for (const auto& hw : sizes) {
    const int H = hw[0], W = hw[1];
    std::vector<float> offs = {0.0f, -0.0f, 0.25f, -0.25f, 0.5f, 1.0f, -1.0f, 1.5f, -1.5f, 2.0f, -2.0f, 1e30f, -1e30f, big, -big, inf, -inf, nan,
                               tiny, -tiny, 2147483648.0f, -2147483648.0f, 4294967296.0f, 16777216.0f, -16777217.0f, 1e10f, -1e10f};
    // per pixel: the offsets that put the sample exactly on -1, H - 1, H (W - 1, W) and one ulp to either side
    std::vector<int> hs = {0, H / 2, H - 1}, ws = {0, W / 2, W - 1};
    if (H <= 40 && W <= 60) {
      hs.clear();
      ws.clear();
      for (int h = 0; h < H; ++h) hs.push_back(h);
      for (int w = 0; w < W; ++w) ws.push_back(w);
    }
    for (int h : hs)
      for (int w : ws)
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) {
            std::vector<float> dys = offs, dxs = offs;
            const float by = (float)(h - 1 + ky), bx = (float)(w - 1 + kx);
            for (float t : {-1.0f, 0.0f, (float)(H - 1), (float)H, (float)(H - 2)})
              for (float d : {t - by, std::nextafterf(t - by, inf), std::nextafterf(t - by, -inf)}) dys.push_back(d);
            for (float t : {-1.0f, 0.0f, (float)(W - 1), (float)W, (float)(W - 2)})
              for (float d : {t - bx, std::nextafterf(t - bx, inf), std::nextafterf(t - bx, -inf)}) dxs.push_back(d);
            if (H * (long long)W > 200) {           // the larger maps: every dy with a few dx and the reverse, not the full product
              for (float dy : dys)
                for (float dx : {0.0f, 0.5f, dxs[dxs.size() - 8], nan, 1e30f}) check(h, w, ky, kx, dy, dx, H, W);
              for (float dx : dxs)
                for (float dy : {0.0f, 0.5f, dys[dys.size() - 8], -inf, -1e30f}) check(h, w, ky, kx, dy, dx, H, W);
            } else {
              for (float dy : dys)
                for (float dx : dxs) check(h, w, ky, kx, dy, dx, H, W);
            }
          }
  }
  std::printf("deform_geom_check: %lld samples, every valid index in range\n", g_checked);
  return 0;
}
