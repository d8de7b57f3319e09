// The data-dependent addressing of the matching stage's similarity and its backward pass (k_mvs_similarity and k_mvs_similarity_grad in mvs.hip), kept apart from the kernels so
// that a plain host program can drive it under a sanitizer (tools/mvs_geom_check.cpp): the map from a reference pixel, a depth hypothesis
// and a view's homography (rot | trans, 12 floats of k_mvs_homography) to the four source pixels the bilinear sample reads and their
// weights.
//
// It restates k_mvs_cost_volume's (mvs.hip) operations in its order: rot (x, y, 1) as an fmaf onto a product plus the third term, the
// three fmaf's with the depth, valid = !(z < 1e-6), the quotient clamped to [-2, size + 1] before floor and the conversion to int (so the
// conversion is defined for every input and a NaN lands on -2, "outside"), tap indices clamped into the map, and the weight of a tap
// outside the map or of an invalid sample exactly 0.  Nothing here reads memory.  Every returned index lies in [0, H W) whatever the
// inputs are: the backward pass scatters to these addresses.
#pragma once

#if defined(__HIPCC__)
#define DINER_GEOM_HD __host__ __device__
#else
#define DINER_GEOM_HD
#endif

#include <math.h>

// One spelling for both compilers: fmaf is the fused multiply-add __fmaf_rn names, and a plain product rounds once like __fmul_rn because
// every build of this file, the library's and the host check's, passes -ffp-contract=off (nothing is contracted behind the source's back).
#define DINER_GEOM_FMA(a, b, c) fmaf(a, b, c)
#define DINER_GEOM_MUL(a, b) ((a) * (b))

namespace diner {

struct MvsTaps {
  int idx[4];       // pixel index y W + x of the taps (y0,x0), (y0,x1), (y1,x0), (y1,x1), each clamped into the map
  float wt[4];      // wx0 wy0, wx1 wy0, wx0 wy1, wx1 wy1; exactly 0 for a tap outside the map and for an invalid sample
};

// hm: rot (row-major 3 x 3) | trans (3); (x, y): the reference pixel; z: the depth hypothesis, any float; 1 <= H, W with H W < 2^31.
DINER_GEOM_HD inline MvsTaps mvs_taps(const float* hm, int x, int y, float z, int H, int W) {
  const float fx = (float)x, fy = (float)y;
  const float rx = DINER_GEOM_FMA(hm[1], fy, DINER_GEOM_MUL(hm[0], fx)) + hm[2];
  const float ry = DINER_GEOM_FMA(hm[4], fy, DINER_GEOM_MUL(hm[3], fx)) + hm[5];
  const float rz = DINER_GEOM_FMA(hm[7], fy, DINER_GEOM_MUL(hm[6], fx)) + hm[8];
  const float px3 = DINER_GEOM_FMA(rx, z, hm[9]), py3 = DINER_GEOM_FMA(ry, z, hm[10]), pz3 = DINER_GEOM_FMA(rz, z, hm[11]);
  const bool valid = !(pz3 < 1e-6f);
  // beyond [-1, size] every tap is outside; the clamp keeps the conversion to int defined and sends NaN to "outside"
  const float sx = fminf(fmaxf(px3 / pz3, -2.0f), (float)W + 1.0f);
  const float sy = fminf(fmaxf(py3 / pz3, -2.0f), (float)H + 1.0f);
  const float x0f = floorf(sx), y0f = floorf(sy);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float tx = sx - x0f, ty = sy - y0f;
  const bool inx0 = x0 >= 0 && x0 < W, inx1 = x0 + 1 >= 0 && x0 + 1 < W;
  const bool iny0 = y0 >= 0 && y0 < H, iny1 = y0 + 1 >= 0 && y0 + 1 < H;
  const float wx0 = (valid && inx0) ? 1.0f - tx : 0.0f, wx1 = (valid && inx1) ? tx : 0.0f;
  const float wy0 = iny0 ? 1.0f - ty : 0.0f, wy1 = iny1 ? ty : 0.0f;
  const int xa = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0), xb = x0 + 1 < 0 ? 0 : (x0 + 1 > W - 1 ? W - 1 : x0 + 1);
  const int ya = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0), yb = y0 + 1 < 0 ? 0 : (y0 + 1 > H - 1 ? H - 1 : y0 + 1);
  MvsTaps t;
  t.idx[0] = ya * W + xa;
  t.idx[1] = ya * W + xb;
  t.idx[2] = yb * W + xa;
  t.idx[3] = yb * W + xb;
  t.wt[0] = DINER_GEOM_MUL(wx0, wy0);
  t.wt[1] = DINER_GEOM_MUL(wx1, wy0);
  t.wt[2] = DINER_GEOM_MUL(wx0, wy1);
  t.wt[3] = DINER_GEOM_MUL(wx1, wy1);
  return t;
}

}  // namespace diner
