// The perceptual network on the device (diner_amd/perceptual.py): the VGG convolution stack behind the reference's two perceptual
// quantities -- the LPIPS score of evaluate_folder (eval_suite.py:52,75-77) and the VGG loss of every shipped training config
// (vggloss.py:59-69) -- as the 3 x 3 convolution of conv2d.hip and four more building blocks, all fp32, activations channels-last
// (N,H,W,C):
//   * k_maxpool2 / k_maxpool2_bwd: MaxPool2d(2, 2), odd sizes floored; the gradient goes to the first maximum of a window in row-major
//     order (torch's CPU max_pool2d), recomputed from the saved input.
//   * k_image_in / k_image_in_bwd: (N,3,H,W) -> channels-last with a per-channel affine, and its adjoint.
//   * k_feature_l1 (+ k_sum_partials): mean |fx - fy| of one tap layer and the gradient plane for the x side.
//   * k_lpips_layer (+ k_sum_partials): unit-normalise over channels, squared difference, dot with the layer's lin weights, spatial mean.
// No floating-point atomics: every sum runs in an order fixed by the sizes alone, the two reductions in double.
#include <cmath>
#include "common.hpp"

namespace diner {
namespace {

// ---- 2 x 2 max-pool --------------------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;

// the first maximum of the window at (2 ho, 2 wo) in row-major order, as torch's CPU kernel keeps it: a later value wins only when it is
// greater, or a NaN
__device__ __forceinline__ int first_max(const float* x, size_t base, size_t row, int C, float* vmax) {
  float best = x[base];
  int at = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const float v = x[base + (k >> 1) * row + (size_t)(k & 1) * C];
    if (v > best || v != v) { best = v; at = k; }
  }
  *vmax = best;
  return at;
}

__global__ __launch_bounds__(kThreads) void k_maxpool2(const float* x, float* y, long long total, int H, int W, int C, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  long long p = i / C;
  const int wo = (int)(p % Wo);
  p /= Wo;
  const int ho = (int)(p % Ho);
  const long long n = p / Ho;
  float v;
  first_max(x, (((size_t)n * H + 2 * ho) * W + 2 * wo) * C + c, (size_t)W * C, C, &v);
  y[i] = v;
}

// one thread per INPUT element: it takes the window's gradient iff it is the window's first maximum; then the optional addend (the loss
// gradient entering at this activation) and the optional ReLU mask (x is the saved post-ReLU activation)
__global__ __launch_bounds__(kThreads) void k_maxpool2_bwd(const float* x, const float* gy, const float* addend, float* gx, long long total,
                                                           int H, int W, int C, int Ho, int Wo, int relu_mask) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  long long p = i / C;
  const int w = (int)(p % W);
  p /= W;
  const int h = (int)(p % H);
  const long long n = p / H;
  float g = 0.0f;
  const int ho = h >> 1, wo = w >> 1;
  if (ho < Ho && wo < Wo) {
    float v;
    const int at = first_max(x, (((size_t)n * H + 2 * ho) * W + 2 * wo) * C + c, (size_t)W * C, C, &v);
    if (at == ((h & 1) << 1 | (w & 1))) g = gy[(((size_t)n * Ho + ho) * Wo + wo) * C + c];
  }
  if (addend) g += addend[i];
  if (relu_mask && !(x[i] > 0.0f)) g = 0.0f;
  gx[i] = g;
}

// ---- image in --------------------------------------------------------------------------------------------------------------------------
struct Affine3 { float shift[3], scale[3]; };

__global__ __launch_bounds__(kThreads) void k_image_in(const float* x, float* y, long long pixels, long long HW, int Cs, Affine3 af) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= pixels) return;
  const long long n = i / HW, p = i % HW;
#pragma unroll
  for (int c = 0; c < 3; ++c) y[(size_t)i * Cs + c] = __fdiv_rn(__fsub_rn(x[((size_t)n * 3 + c) * HW + p], af.shift[c]), af.scale[c]);
  if (Cs == 4) y[(size_t)i * 4 + 3] = 0.0f;
}

__global__ __launch_bounds__(kThreads) void k_image_in_bwd(const float* g, float* gx, long long pixels, long long HW, int Cs, Affine3 af) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= pixels) return;
  const long long n = i / HW, p = i % HW;
#pragma unroll
  for (int c = 0; c < 3; ++c) gx[((size_t)n * 3 + c) * HW + p] = __fdiv_rn(g[(size_t)i * Cs + c], af.scale[c]);
}

// ---- reductions in double, fixed order -------------------------------------------------------------------------------------------------
constexpr int kMaxBlocks = 1024;

int l1_blocks(long long n) {
  const long long b = (n + kThreads - 1) / kThreads;
  return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

__global__ __launch_bounds__(kThreads) void k_feature_l1(const float* fx, const float* fy, long long n, float gscale, int mask_by_fx, float* grad,
                                                         double* partial) {
  __shared__ double sh[4];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const float a = fx[i];
    const double d = (double)a - (double)fy[i];          // exact
    s += fabs(d);
    if (grad) {
      float g = d > 0.0 ? gscale : (d < 0.0 ? -gscale : 0.0f);
      if (mask_by_fx && !(a > 0.0f)) g = 0.0f;
      grad[i] = g;
    }
  }
  s = block_sum_d<kThreads / 64>(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[blockIdx.x] (+)= (sum of the block's `count` partials, lane-strided then over the wave) / denom
__global__ __launch_bounds__(64) void k_sum_partials(const double* partial, int count, double denom, int accumulate, double* out) {
  const double* p = partial + (size_t)blockIdx.x * count;
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += 64) s += p[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) {
    const double v = s / denom;
    out[blockIdx.x] = accumulate ? out[blockIdx.x] + v : v;
  }
}

constexpr int kLpipsMaxBlocks = 256;
int lpips_blocks(long long HW) {
  const long long b = (HW + 3) / 4;
  return (int)(b < kLpipsMaxBlocks ? b : kLpipsMaxBlocks);
}

// one wave per pixel, lanes over channels; grid (blocks, N): image blockIdx.y, so an image's sums do not depend on its place in the batch
__global__ __launch_bounds__(kThreads) void k_lpips_layer(const float* fx, const float* fy, const float* lin, long long HW, int C,
                                                          double* partial) {
  __shared__ double sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t img = (size_t)blockIdx.y * HW;
  double total = 0.0;
  for (long long p = (long long)blockIdx.x * 4 + wave; p < HW; p += (long long)gridDim.x * 4) {
    const float* px = fx + (img + p) * C;
    const float* py = fy + (img + p) * C;
    double sx = 0.0, sy = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double a = px[c], b = py[c];
      sx += a * a;
      sy += b * b;
    }
    const double nx = sqrt(wave_sum_d(sx)) + 1e-10, ny = sqrt(wave_sum_d(sy)) + 1e-10;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double d = (double)px[c] / nx - (double)py[c] / ny;
      s += (double)lin[c] * (d * d);
    }
    total += wave_sum_d(s);
  }
  total = waves_sum_d<kThreads / 64>(total, sh);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

inline unsigned blocks_for(long long total) { return (unsigned)((total + kThreads - 1) / kThreads); }
constexpr long long kMaxElems = (1LL << 31) * (long long)kThreads - 1;      // one thread per element, grid.x < 2^31

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" int diner_maxpool2_f32(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  const int rc = check_nhwc("maxpool2", N, H, W, C);
  if (rc) return rc;
  DINER_CHECK_ARG(H >= 2 && W >= 2, "maxpool2: H, W = %d, %d (each must be >= 2)", H, W);
  DINER_CHECK_ARG(x && y, "maxpool2: null pointer argument");
  const int Ho = H / 2, Wo = W / 2;
  const long long total = (long long)N * Ho * Wo * C;
  DINER_CHECK_ARG(total <= kMaxElems, "maxpool2: too many elements");
  hipLaunchKernelGGL(k_maxpool2, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, x, y, total, H, W, C, Ho, Wo);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_maxpool2_bwd_f32(const float* x, const float* gy, const float* addend, int relu_mask, float* gx, int N, int H, int W, int C,
                                      void* stream) {
  const int rc = check_nhwc("maxpool2_bwd", N, H, W, C);
  if (rc) return rc;
  DINER_CHECK_ARG(H >= 2 && W >= 2, "maxpool2_bwd: H, W = %d, %d (each must be >= 2)", H, W);
  DINER_CHECK_ARG(x && gy && gx, "maxpool2_bwd: null pointer argument");
  const long long total = (long long)N * H * W * C;
  DINER_CHECK_ARG(total <= kMaxElems, "maxpool2_bwd: too many elements");
  hipLaunchKernelGGL(k_maxpool2_bwd, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, x, gy, addend, gx, total, H, W, C, H / 2,
                     W / 2, relu_mask != 0);
  DINER_LAUNCH_OK();
  return 0;
}

static int make_affine(const char* who, const float* shift, const float* scale, Affine3* af) {
  DINER_CHECK_ARG(scale != nullptr, "%s: null pointer argument (scale)", who);
  for (int c = 0; c < 3; ++c) {
    af->shift[c] = shift ? shift[c] : 0.0f;
    af->scale[c] = scale[c];
    DINER_CHECK_ARG(std::isfinite(af->shift[c]) && std::isfinite(scale[c]) && scale[c] != 0.0f, "%s: channel %d: shift %g, scale %g (need finite, scale != 0)",
                    who, c, (double)af->shift[c], (double)scale[c]);
  }
  return 0;
}

extern "C" int diner_image_in_f32(const float* x, const float* shift, const float* scale, float* y, int N, int H, int W, int Cs, void* stream) {
  int rc = check_nhwc("image_in", N, H, W, 4);
  if (rc) return rc;
  DINER_CHECK_ARG(Cs == 3 || Cs == 4, "image_in: Cs = %d output channels (3, or 4 with a zero fourth)", Cs);
  DINER_CHECK_ARG(x && shift && y, "image_in: null pointer argument");
  Affine3 af;
  rc = make_affine("image_in", shift, scale, &af);
  if (rc) return rc;
  const long long HW = (long long)H * W, pixels = N * HW;
  hipLaunchKernelGGL(k_image_in, dim3(blocks_for(pixels)), dim3(kThreads), 0, (hipStream_t)stream, x, y, pixels, HW, Cs, af);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_image_in_bwd_f32(const float* g, const float* scale, float* gx, int N, int H, int W, int Cs, void* stream) {
  int rc = check_nhwc("image_in_bwd", N, H, W, 4);
  if (rc) return rc;
  DINER_CHECK_ARG(Cs == 3 || Cs == 4, "image_in_bwd: Cs = %d gradient channels (3 or 4)", Cs);
  DINER_CHECK_ARG(g && gx, "image_in_bwd: null pointer argument");
  Affine3 af;
  rc = make_affine("image_in_bwd", nullptr, scale, &af);
  if (rc) return rc;
  const long long HW = (long long)H * W, pixels = N * HW;
  hipLaunchKernelGGL(k_image_in_bwd, dim3(blocks_for(pixels)), dim3(kThreads), 0, (hipStream_t)stream, g, gx, pixels, HW, Cs, af);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" size_t diner_feature_l1_workspace_bytes(long long n) { return n < 1 ? 0 : (size_t)l1_blocks(n) * sizeof(double); }

extern "C" int diner_feature_l1_f32(const float* fx, const float* fy, long long n, double weight, int mask_by_fx, float* grad, void* workspace,
                                    double* out, void* stream) {
  DINER_CHECK_ARG(n >= 1, "feature_l1: n = %lld elements (need >= 1)", n);
  DINER_CHECK_ARG(std::isfinite(weight), "feature_l1: weight %g is not finite", weight);
  DINER_CHECK_ARG(fx && fy && workspace && out, "feature_l1: null pointer argument");
  const int blocks = l1_blocks(n);
  hipLaunchKernelGGL(k_feature_l1, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, fx, fy, n, (float)(weight / (double)n),
                     mask_by_fx != 0, grad, (double*)workspace);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, blocks, (double)n, 0, out);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" size_t diner_lpips_layer_workspace_bytes(int N, long long HW) {
  return (N < 1 || HW < 1) ? 0 : (size_t)N * lpips_blocks(HW) * sizeof(double);
}

extern "C" int diner_lpips_layer_f32(const float* fx, const float* fy, const float* lin, int N, long long HW, int C, int accumulate, void* workspace,
                                     double* out, void* stream) {
  DINER_CHECK_ARG(N >= 1 && N <= 65535, "lpips_layer: N = %d images (need 1 .. 65535)", N);
  DINER_CHECK_ARG(HW >= 1 && C >= 1 && HW <= (1LL << 40) / C / N, "lpips_layer: HW = %lld pixels, C = %d channels", HW, C);
  DINER_CHECK_ARG(fx && fy && lin && workspace && out, "lpips_layer: null pointer argument");
  const int blocks = lpips_blocks(HW);
  hipLaunchKernelGGL(k_lpips_layer, dim3((unsigned)blocks, (unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, fx, fy, lin, HW, C,
                     (double*)workspace);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_sum_partials, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, blocks, (double)HW,
                     accumulate != 0, out);
  DINER_LAUNCH_OK();
  return 0;
}
