// The image encoder's trunk on the device (diner_amd/encoder.py): what SpatialEncoder.forward (image_encoder.py of the reference, :225-291)
// needs beside the convolutions of conv2d.hip, all fp32, activations channels-last (N,H,W,C):
//   * k_maxpool3s2: MaxPool2d(3, 2, 1); the input has a channel stride (it reads the stem's output inside the latent).
//   * k_encoder_input: (N,3,H,W) -> channels-last, replication-padded, with the positional-encoding ring channels and zero channels
//     behind them (the stem reads 24 channels, not 21: float4 loads).
//   * k_pyramid_level: bilinear align_corners=True resampling of one pyramid level into its channel slice of the latent.
// Every output is computed in an order the shape alone fixes.
#include <cmath>
#include "common.hpp"

namespace diner {
namespace {

// ---- element-wise kernels: one thread per output element -------------------------------------------------------------------------------
constexpr int kThreads = 256;

// torch's MaxPool2d(3, 2, 1): the padding is -inf (it never wins); a later value replaces the maximum when it is greater, or a NaN (torch's
// CPU kernel), so a NaN in the window propagates
__global__ __launch_bounds__(kThreads) void k_maxpool3s2(const float* x, float* y, long long total, int H, int W, int C, int ldx, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  long long p = i / C;
  const int wo = (int)(p % Wo);
  p /= Wo;
  const int ho = (int)(p % Ho);
  const long long n = p / Ho;
  float best = -INFINITY;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int h = 2 * ho - 1 + dy;
    if (h < 0 || h >= H) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int w = 2 * wo - 1 + dx;
      if (w < 0 || w >= W) continue;
      const float v = x[(((size_t)n * H + h) * W + w) * ldx + c];
      if (v > best || v != v) best = v;
    }
  }
  y[i] = best;
}

// y (N, H + 2 p, W + 2 p, C): channels 0 .. 2 the image, replication-padded; 3 .. 3 + Cr - 1 the ring plane (H + 2 p, W + 2 p, Cr), the
// same for every image; the rest zero
__global__ __launch_bounds__(kThreads) void k_encoder_input(const float* x, const float* ring, float* y, long long total, int H, int W, int pad,
                                                            int Cr, int C) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int Hp = H + 2 * pad, Wp = W + 2 * pad;
  const int c = (int)(i % C);
  long long p = i / C;
  const int wp = (int)(p % Wp);
  p /= Wp;
  const int hp = (int)(p % Hp);
  const long long n = p / Hp;
  float v = 0.0f;
  if (c < 3) {
    const int h = min(max(hp - pad, 0), H - 1), w = min(max(wp - pad, 0), W - 1);
    v = x[(((size_t)n * 3 + c) * H + h) * W + w];
  } else if (c < 3 + Cr) {
    v = ring[((size_t)hp * Wp + wp) * Cr + (c - 3)];
  }
  y[i] = v;
}

// bilinear resampling with align_corners=True: source coordinate = dst * (in - 1) / (out - 1) (scale 0 when out == 1), weights (1 - l, l).
// The coordinate, the weights and the four products are evaluated in double and the result is rounded once: a memory-bound kernel pays
// nothing for it, and the output is within half an ulp of the exact interpolant.  One thread per V channels of one output pixel (V = 4:
// 16-byte loads and stores, where the channel counts, the offset and the pointers allow them); the output row is blockIdx.y and the image
// blockIdx.z, which leaves one 32-bit division for the index
template <int V>
__global__ __launch_bounds__(kThreads) void k_pyramid_level(const float* x, float* y, unsigned row_elems, int h, int w, int c, int Wf, int Ctot, int c0,
                                                            double sh, double sw) {
  const unsigned j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= row_elems) return;
  const unsigned cv = (unsigned)c / V;
  const int xo = (int)(j / cv), ch = (int)(j % cv) * V, yo = (int)blockIdx.y, Hf = (int)gridDim.y;
  const float* src = x + (size_t)blockIdx.z * h * w * c + ch;
  float* dst = y + (((size_t)blockIdx.z * Hf + yo) * Wf + xo) * Ctot + c0 + ch;
  float v[4][V];
  auto load = [&](float* to, int yy, int xx) {
    const float* p = src + ((size_t)yy * w + xx) * c;
    if constexpr (V == 4) {
      const v4f t = *reinterpret_cast<const v4f*>(p);
      to[0] = t[0]; to[1] = t[1]; to[2] = t[2]; to[3] = t[3];
    } else {
      to[0] = p[0];
    }
  };
  float out[V];
  if (h == Hf && w == Wf) {                // a copy, bit for bit
    load(out, yo, xo);
  } else {
    const double fy = sh * yo, fx = sw * xo;
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const double ly = fy - y0, lx = fx - x0;
    load(v[0], y0, x0);
    load(v[1], y0, x1);
    load(v[2], y1, x0);
    load(v[3], y1, x1);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const double top = (1.0 - lx) * (double)v[0][k] + lx * (double)v[1][k], bot = (1.0 - lx) * (double)v[2][k] + lx * (double)v[3][k];
      out[k] = (float)((1.0 - ly) * top + ly * bot);
    }
  }
  if constexpr (V == 4) {
    *reinterpret_cast<v4f*>(dst) = (v4f){out[0], out[1], out[2], out[3]};
  } else {
    dst[0] = out[0];
  }
}

inline unsigned blocks_for(long long total) { return (unsigned)((total + kThreads - 1) / kThreads); }
constexpr long long kMaxElems = (1LL << 31) * (long long)kThreads - 1;      // one thread per element, grid.x < 2^31

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" int diner_maxpool3s2_f32(const float* x, float* y, int N, int H, int W, int C, int ldx, void* stream) {
  const int rc = check_nhwc("maxpool3s2", N, H, W, C);
  if (rc) return rc;
  DINER_CHECK_ARG(ldx >= C && (long long)N * H * W <= (1LL << 40) / ldx, "maxpool3s2: ldx = %d (the input's channel stride, >= C = %d)", ldx, C);
  DINER_CHECK_ARG(x && y, "maxpool3s2: null pointer argument");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long total = (long long)N * Ho * Wo * C;
  DINER_CHECK_ARG(total <= kMaxElems, "maxpool3s2: too many elements");
  hipLaunchKernelGGL(k_maxpool3s2, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, x, y, total, H, W, C, ldx, Ho, Wo);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_encoder_input_f32(const float* x, const float* ring, float* y, int N, int H, int W, int pad, int Cring, int C, void* stream) {
  DINER_CHECK_ARG(pad >= 0 && pad <= (1 << 20), "encoder_input: pad = %d (need 0 .. 2^20)", pad);
  DINER_CHECK_ARG(Cring >= 0 && C >= 3 && Cring <= C - 3, "encoder_input: C = %d output channels do not hold 3 + Cring = %d ring channels", C, Cring);
  DINER_CHECK_ARG(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24), "encoder_input: N, H, W, C = %d, %d, %d, %d (each must be >= 1)", N, H, W, C);
  const int rc = check_nhwc("encoder_input", N, H + 2 * pad, W + 2 * pad, C);
  if (rc) return rc;
  DINER_CHECK_ARG(x && y && (ring || Cring == 0), "encoder_input: null pointer argument");
  const long long total = (long long)N * (H + 2 * pad) * (W + 2 * pad) * C;
  DINER_CHECK_ARG(total <= kMaxElems, "encoder_input: too many elements");
  hipLaunchKernelGGL(k_encoder_input, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, x, ring, y, total, H, W, pad, Cring, C);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_pyramid_level_f32(const float* x, float* y, int N, int h, int w, int c, int Hf, int Wf, int Ctot, int c0, void* stream) {
  int rc = check_nhwc("pyramid_level", N, h, w, c);
  if (rc) return rc;
  rc = check_nhwc("pyramid_level", N, Hf, Wf, Ctot);
  if (rc) return rc;
  DINER_CHECK_ARG(c0 >= 0 && c <= Ctot - c0, "pyramid_level: channels %d .. %d do not fit a latent of %d channels", c0, c0 + c - 1, Ctot);
  DINER_CHECK_ARG(x && y, "pyramid_level: null pointer argument");
  DINER_CHECK_ARG(N <= 65535 && Hf <= 65535, "pyramid_level: N = %d images, Hf = %d rows (at most 65535 each a call)", N, Hf);
  DINER_CHECK_ARG((long long)Wf * c < (1LL << 31), "pyramid_level: too many elements in a row of %d pixels x %d channels", Wf, c);
  const double sh = Hf > 1 ? (double)(h - 1) / (double)(Hf - 1) : 0.0, sw = Wf > 1 ? (double)(w - 1) / (double)(Wf - 1) : 0.0;
  const bool vec = ((c | Ctot | c0) & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const unsigned row_elems = (unsigned)Wf * (unsigned)(vec ? c / 4 : c);
  const dim3 grid((row_elems + kThreads - 1) / kThreads, (unsigned)Hf, (unsigned)N);
  if (vec)
    hipLaunchKernelGGL(k_pyramid_level<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, y, row_elems, h, w, c, Wf, Ctot, c0, sh, sw);
  else
    hipLaunchKernelGGL(k_pyramid_level<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, y, row_elems, h, w, c, Wf, Ctot, c0, sh, sw);
  DINER_LAUNCH_OK();
  return 0;
}
