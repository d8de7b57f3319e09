// A host program around diner::deform_corner_grads (diner_amd/csrc/deform_geom.hpp), the addressing and the weight derivatives of the
// deformable convolution's backward pass (deform_grad.hip).  Built for the host alone, with deform_geom_check.cpp's line,
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/deform_grad_geom_check.cpp
// (tests/test_deform_grad_cpu.py does that), it feeds the function the adversarial offsets of that program -- huge, infinite, NaN, exactly
// -1, exactly H - 1, exactly H, one ulp to either side of each -- and checks that
//   * its corners are deform_corners()' of the same arguments, bit for bit (so a valid index is in range: that program's finding);
//   * a sample the rule calls outside has eight derivatives that are exactly 0 (+0 or -0, never NaN);
//   * otherwise they are (-hx, -lx, hx, lx) by the row and (-hy, hy, -ly, ly) by the column of the fp32 hy, ly, hx, lx, finite and in
//     [-1, 1], and each of the two sets sums to exactly 0;
//   * at an exactly integer coordinate the derivative is the right-sided difference: the weight of the corner one further (ly = 0, so the
//     corners of row y0 + 1 carry weight 0 and derivative + hx, + lx).
// Prints the number of samples checked and exits 0, or prints the first violation and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  const diner::DeformCornerGrads g = diner::deform_corner_grads(h, w, ky, kx, dy, dx, H, W);
  const diner::DeformCorners c = diner::deform_corners(h, w, ky, kx, dy, dx, H, W);
  ++g_checked;
  if (std::memcmp(g.c.idx, c.idx, sizeof c.idx) != 0 || std::memcmp(g.c.wt, c.wt, sizeof c.wt) != 0 || g.c.valid != c.valid)
    fail("the corners differ from deform_corners()", h, w, ky, kx, dy, dx, H, W);
  const float pyf = (float)(h - 1 + ky) + dy, pxf = (float)(w - 1 + kx) + dx;
  const double py = pyf, px = pxf;
  const bool outside = std::isnan(py) || std::isnan(px) || py <= -1.0 || py >= (double)H || px <= -1.0 || px >= (double)W;
  if (outside) {
    for (int i = 0; i < 4; ++i)
      if (!(g.gy[i] == 0.0f && g.gx[i] == 0.0f)) fail("an outside sample carries a derivative", h, w, ky, kx, dy, dx, H, W);
    return;
  }
  const double y0 = std::floor(py), x0 = std::floor(px);
  const float ly = pyf - (float)y0, lx = pxf - (float)x0, hy = 1.0f - ly, hx = 1.0f - lx;
  const float want_gy[4] = {-hx, -lx, hx, lx}, want_gx[4] = {-hy, hy, -ly, ly};
  for (int i = 0; i < 4; ++i) {
    if (!(g.gy[i] >= -1.0f && g.gy[i] <= 1.0f && g.gx[i] >= -1.0f && g.gx[i] <= 1.0f))
      fail("a derivative is outside [-1, 1]", h, w, ky, kx, dy, dx, H, W);
    if (g.gy[i] != want_gy[i] || g.gx[i] != want_gx[i]) fail("a derivative differs from the rule", h, w, ky, kx, dy, dx, H, W);
  }
  if (g.gy[0] + g.gy[2] != 0.0f || g.gy[1] + g.gy[3] != 0.0f || g.gx[0] + g.gx[1] != 0.0f || g.gx[2] + g.gx[3] != 0.0f)
    fail("a pair of derivatives does not cancel", h, w, ky, kx, dy, dx, H, W);
  if (py == y0 && (g.gy[2] != hx || g.gy[3] != lx || c.wt[2] != 0.0f || c.wt[3] != 0.0f))
    fail("an integer row is not the right-sided difference", h, w, ky, kx, dy, dx, H, W);
  if (px == x0 && (g.gx[1] != hy || g.gx[3] != ly || c.wt[1] != 0.0f || c.wt[3] != 0.0f))
    fail("an integer column is not the right-sided difference", h, w, ky, kx, dy, dx, H, W);
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float big = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
  const int sizes[][2] = {{1, 1}, {1, 7}, {5, 1}, {4, 6}, {9, 13}, {36, 52}, {256, 320}, {3, 46340}, {46340, 3}, {16384, 16384}};
  const std::vector<float> offs = {0.0f, -0.0f, 0.25f, -0.25f, 0.5f, 1.0f, -1.0f, 1.5f, -1.5f, 2.0f, -2.0f, 1e30f, -1e30f, big, -big, inf, -inf,
                                   nan, tiny, -tiny, 2147483648.0f, -2147483648.0f, 4294967296.0f, 16777216.0f, -16777217.0f, 1e10f, -1e10f};
  for (const auto& hw : sizes) {
    const int H = hw[0], W = hw[1];
    const bool small = H * (long long)W <= 200;
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
            // besides the common offsets: those that put this tap exactly on -1, 0, size - 2, size - 1, size, and one ulp to either side
            std::vector<float> dys = offs, dxs = offs;
            const float by = (float)(h - 1 + ky), bx = (float)(w - 1 + kx);
            for (float t : {-1.0f, 0.0f, (float)(H - 2), (float)(H - 1), (float)H})
              for (float d : {t - by, std::nextafterf(t - by, inf), std::nextafterf(t - by, -inf)}) dys.push_back(d);
            for (float t : {-1.0f, 0.0f, (float)(W - 2), (float)(W - 1), (float)W})
              for (float d : {t - bx, std::nextafterf(t - bx, inf), std::nextafterf(t - bx, -inf)}) dxs.push_back(d);
            if (small) {
              for (float dy : dys)
                for (float dx : dxs) check(h, w, ky, kx, dy, dx, H, W);
            } else {                                  // the larger maps: every dy with a few dx and the reverse
              for (float dy : dys)
                for (float dx : {0.0f, 0.5f, dxs[dxs.size() - 5], nan, 1e30f}) check(h, w, ky, kx, dy, dx, H, W);
              for (float dx : dxs)
                for (float dy : {0.0f, 0.5f, dys[dys.size() - 5], -inf, -1e30f}) check(h, w, ky, kx, dy, dx, H, W);
            }
          }
  }
  std::printf("deform_grad_geom_check: %lld samples, outside samples carry exact zeros\n", g_checked);
  return 0;
}
