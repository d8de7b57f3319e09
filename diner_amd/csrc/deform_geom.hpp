// The data-dependent addressing of the modulated deformable 3 x 3 convolution (deform.hip), kept apart from the kernel so that a plain
// host program can drive it under a sanitizer (tools/deform_geom_check.cpp): the map from an output pixel, a tap and the tap's learned
// offset to the four input pixels the bilinear sample reads, their weights and which of them exist.
//
// torchvision's deform_conv2d (stride 1, padding 1, dilation 1) samples input channel c of tap k = 3 ky + kx at
//   py = (h - 1 + ky) + dy,   px = (w - 1 + kx) + dx
// (the integer part summed first, then one fp32 addition) with its bilinear_interpolate:
//   0 when py <= -1, py >= H, px <= -1 or px >= W; otherwise y0 = floor(py), ly = py - y0, hy = 1 - ly (columns likewise), a corner
//   outside [0, H - 1] x [0, W - 1] contributes 0, and the value is hy hx v00 + hy lx v01 + ly hx v10 + ly lx v11.
// Nothing here reads memory.  Every comparison is written so that a NaN coordinate fails it and lands on "outside"; the float -> int
// conversion happens only after the coordinate is known to lie in (-1, H) x (-1, W), so huge offsets and infinities never reach it.
#pragma once

#if defined(__HIPCC__)
#define DINER_GEOM_HD __host__ __device__
#else
#define DINER_GEOM_HD
#endif

#include <math.h>

namespace diner {

struct DeformCorners {
  int idx[4];       // pixel index y W + x of the corners (y0,x0), (y0,x1), (y1,x0), (y1,x1); 0 where the corner is not valid
  float wt[4];      // hy hx, hy lx, ly hx, ly lx; 0 where the whole sample is outside
  unsigned valid;   // bit i: corner i lies inside the image and idx[i] may be read
};

// h, w: the output pixel (0 <= h < H, 0 <= w < W); ky, kx in 0 .. 2; dy, dx: any float, finite or not; 1 <= H, W <= 2^24 (exact in fp32)
// with H W < 2^31.
DINER_GEOM_HD inline DeformCorners deform_corners(int h, int w, int ky, int kx, float dy, float dx, int H, int W) {
  DeformCorners c;
  for (int i = 0; i < 4; ++i) {
    c.idx[i] = 0;
    c.wt[i] = 0.0f;
  }
  c.valid = 0u;
  const float py = (float)(h - 1 + ky) + dy, px = (float)(w - 1 + kx) + dx;
  // inside <=> -1 < p < size; written positively, so that a NaN is outside
  if (!(py > -1.0f && py < (float)H && px > -1.0f && px < (float)W)) return c;
  // -1 < p < size here; the clamp states the range the conversion below relies on
  const float fy = fminf(fmaxf(floorf(py), -1.0f), (float)(H - 1)), fx = fminf(fmaxf(floorf(px), -1.0f), (float)(W - 1));
  const int y0 = (int)fy, x0 = (int)fx, y1 = y0 + 1, x1 = x0 + 1;
  const float ly = py - fy, lx = px - fx, hy = 1.0f - ly, hx = 1.0f - lx;
  c.wt[0] = hy * hx;
  c.wt[1] = hy * lx;
  c.wt[2] = ly * hx;
  c.wt[3] = ly * lx;
  const bool y0in = y0 >= 0 && y0 <= H - 1, y1in = y1 >= 0 && y1 <= H - 1;
  const bool x0in = x0 >= 0 && x0 <= W - 1, x1in = x1 >= 0 && x1 <= W - 1;
  if (y0in && x0in) { c.valid |= 1u; c.idx[0] = y0 * W + x0; }
  if (y0in && x1in) { c.valid |= 2u; c.idx[1] = y0 * W + x1; }
  if (y1in && x0in) { c.valid |= 4u; c.idx[2] = y1 * W + x0; }
  if (y1in && x1in) { c.valid |= 8u; c.idx[3] = y1 * W + x1; }
  return c;
}

// The same sample with the derivatives of its four weights by the coordinate (deform_grad.hip, tools/deform_grad_geom_check.cpp):
//   d wt / d py = (-hx, -lx, hx, lx),   d wt / d px = (-hy, hy, -ly, ly)
// torchvision's rule (its get_coordinate_weight), which is also what autograd through floor() gives: at an exactly integer coordinate the
// right-sided difference.  c is deform_corners() of the same arguments, bit for bit.  A sample that lies outside -- a NaN, an infinite or
// a huge offset included -- has every derivative exactly 0, and no non-finite number is ever formed from a finite coordinate.
struct DeformCornerGrads {
  DeformCorners c;
  float gy[4];      // d wt[i] / d py; 0 where the whole sample is outside
  float gx[4];      // d wt[i] / d px
};

DINER_GEOM_HD inline DeformCornerGrads deform_corner_grads(int h, int w, int ky, int kx, float dy, float dx, int H, int W) {
  DeformCornerGrads g;
  g.c = deform_corners(h, w, ky, kx, dy, dx, H, W);
  for (int i = 0; i < 4; ++i) {
    g.gy[i] = 0.0f;
    g.gx[i] = 0.0f;
  }
  const float py = (float)(h - 1 + ky) + dy, px = (float)(w - 1 + kx) + dx;
  if (!(py > -1.0f && py < (float)H && px > -1.0f && px < (float)W)) return g;
  const float fy = fminf(fmaxf(floorf(py), -1.0f), (float)(H - 1)), fx = fminf(fmaxf(floorf(px), -1.0f), (float)(W - 1));
  const float ly = py - fy, lx = px - fx, hy = 1.0f - ly, hx = 1.0f - lx;
  g.gy[0] = -hx; g.gy[1] = -lx; g.gy[2] = hx; g.gy[3] = lx;
  g.gx[0] = -hy; g.gx[1] = hy; g.gx[2] = -ly; g.gx[3] = ly;
  return g;
}

}  // namespace diner
