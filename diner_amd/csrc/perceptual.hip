// The perceptual network on the device (diner_amd/perceptual.py): the VGG convolution stack behind the reference's two perceptual
// quantities -- the LPIPS score of evaluate_folder (eval_suite.py:52,75-77) and the VGG loss of every shipped training config
// (vggloss.py:59-69) -- as five building blocks, all fp32, activations channels-last (N,H,W,C):
//   * k_conv3x3: 3 x 3 convolution, stride 1, zero padding 1, as an implicit GEMM on the fp32-input MFMA (v_mfma_f32_16x16x4_f32, bit
//     for bit an fmaf chain): pixels x Cout accumulators, K = 9 Cin.  With the second packed weight set (taps flipped, Cin and Cout
//     swapped) the same kernel is the data gradient; its epilogue then adds the loss gradient that enters at a tap layer and applies the
//     ReLU mask of the saved activation.  The weights are frozen: there is no weight gradient.
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

typedef float v4f __attribute__((ext_vector_type(4)));

// ---- the convolution -------------------------------------------------------------------------------------------------------------------
// A workgroup (four waves) computes an 8 x 16 pixel tile of one image for 64 output channels.  One tile row = 16 pixels = the 16 rows of
// one MFMA tile, so wave w owns rows 2 w, 2 w + 1 (two M tiles) x four N tiles: 32 accumulator registers.  Per chunk of 8 input channels
// the workgroup stages the 10 x 18 pixel patch (tile + one-pixel halo, zeros outside the image and beyond Cin) and the chunk's
// 9 x 8 x 64 weights in LDS, then runs 9 taps x 2 k-steps x 8 MFMAs per wave between two barriers, the next chunk's loads in flight
// meanwhile.  K order of every output: chunk, tap, channel -- the same whatever the tile or the image's place in the batch.
constexpr int kTH = 8, kTW = 16;
constexpr int kBN = DINER_CONV3X3_COUT_TILE;      // 64
constexpr int kCK = DINER_CONV3X3_CIN_CHUNK;      // 8
constexpr int kPS = kCK + 4;        // LDS words per patch pixel: 12 p + k (16 pixels x 4 k of one operand read) covers the 64 banks once
constexpr int kPH = kTH + 2, kPW = kTW + 2;
constexpr int kWS = kBN + 16;       // LDS words per weight row: the four k rows of one operand read start 16 banks apart
constexpr int kConvThreads = 256;

struct ConvArgs {
  const float* x;        // (N,H,W,Cin)
  const float* w;        // packed [ceil(Cin / 8)][9][8][CoutPad], zeros beyond Cin and Cout
  const float* bias;     // CoutPad or null
  const float* addend;   // (N,H,W,Cout) or null: added before the mask
  const float* mask;     // (N,H,W,Cout) or null: the output is zero where !(mask > 0)
  float* y;              // (N,H,W,Cout)
  int H, W, Cin, Cout, CoutPad, tiles_w, relu;
};

__global__ __launch_bounds__(kConvThreads) void k_conv3x3(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float Xs[kPH * kPW * kPS];
  __shared__ __attribute__((aligned(16))) float Ws[9 * kCK * kWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = ((int)blockIdx.x / a.tiles_w) * kTH, w0 = ((int)blockIdx.x % a.tiles_w) * kTW, n0 = (int)blockIdx.y * kBN;
  const size_t img = (size_t)blockIdx.z * a.H * a.W;       // first pixel of this image: a tile never leaves it
  const float* x = a.x + img * a.Cin;
  const int lc = lane & 15, lk = lane >> 4;
  v4f acc[2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float b = a.bias ? a.bias[n0 + 16 * j + lc] : 0.0f;          // D layout: column lane & 15 in all four registers
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i][j] = (v4f){b, b, b, b};
  }
  const bool vec = (a.Cin & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  const int chunks = (a.Cin + kCK - 1) / kCK;
  // Chunk c + 1 travels from global memory into registers while chunk c's MFMAs run, and moves into LDS behind the barrier that ends them:
  // a small image gives each CU one workgroup, and nothing else would hide the loads.
  constexpr int kPV = (kPH * kPW * 2 + kConvThreads - 1) / kConvThreads;        // float4 patch loads per thread (vector path): 2
  constexpr int kPE = (kPH * kPW * kCK + kConvThreads - 1) / kConvThreads;      // scalar patch loads per thread: 6
  constexpr int kWV = (9 * kCK * (kBN / 4) + kConvThreads - 1) / kConvThreads;  // float4 weight loads per thread: 5
  v4f xv[kPV], wv[kWV];
  float xe[kPE];
  auto fetch = [&](int c) {
    const int c0 = c * kCK;
    if (vec) {
#pragma unroll
      for (int u = 0; u < kPV; ++u) {
        const int e = tid + kConvThreads * u, p = e >> 1, q = e & 1;
        const int h = h0 + p / kPW - 1, w = w0 + p % kPW - 1;
        xv[u] = (v4f){0.f, 0.f, 0.f, 0.f};
        if (e < kPH * kPW * 2 && h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + 4 * q < a.Cin)
          xv[u] = *reinterpret_cast<const v4f*>(x + ((size_t)h * a.W + w) * a.Cin + c0 + 4 * q);
      }
    } else {
#pragma unroll
      for (int u = 0; u < kPE; ++u) {
        const int e = tid + kConvThreads * u, p = e >> 3, k = e & 7;
        const int h = h0 + p / kPW - 1, w = w0 + p % kPW - 1;
        xe[u] = 0.0f;
        if (e < kPH * kPW * kCK && h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + k < a.Cin) xe[u] = x[((size_t)h * a.W + w) * a.Cin + c0 + k];
      }
    }
    const float* wsrc = a.w + (size_t)c * 9 * kCK * a.CoutPad + n0;
#pragma unroll
    for (int u = 0; u < kWV; ++u) {
      const int e = tid + kConvThreads * u, r = e >> 4, q = e & 15;
      if (e < 9 * kCK * (kBN / 4)) wv[u] = *reinterpret_cast<const v4f*>(wsrc + (size_t)r * a.CoutPad + 4 * q);
    }
  };
  auto stash = [&]() {
    if (vec) {
#pragma unroll
      for (int u = 0; u < kPV; ++u) {
        const int e = tid + kConvThreads * u;
        if (e < kPH * kPW * 2) *reinterpret_cast<v4f*>(&Xs[(e >> 1) * kPS + 4 * (e & 1)]) = xv[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < kPE; ++u) {
        const int e = tid + kConvThreads * u;
        if (e < kPH * kPW * kCK) Xs[(e >> 3) * kPS + (e & 7)] = xe[u];
      }
    }
#pragma unroll
    for (int u = 0; u < kWV; ++u) {
      const int e = tid + kConvThreads * u;
      if (e < 9 * kCK * (kBN / 4)) *reinterpret_cast<v4f*>(&Ws[(e >> 4) * kWS + 4 * (e & 15)]) = wv[u];
    }
  };
  fetch(0);
  for (int c = 0; c < chunks; ++c) {
    stash();
    __syncthreads();
    if (c + 1 < chunks) fetch(c + 1);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ky = t / 3, kx = t % 3;
#pragma unroll
      for (int kk = 0; kk < kCK; kk += 4) {
        float av[2], bv[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) av[i] = Xs[((2 * wave + i + ky) * kPW + lc + kx) * kPS + kk + lk];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = Ws[(t * kCK + kk + lk) * kWS + 16 * j + lc];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // D layout: lane holds rows (pixels of the tile row) 4 (lane >> 4) .. + 3 of column (output channel) lane & 15
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int h = h0 + 2 * wave + i;
    if (h >= a.H) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + 16 * j + lc;
      if (n >= a.Cout) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int w = w0 + 4 * lk + r;
        if (w >= a.W) continue;
        const size_t at = (img + (size_t)h * a.W + w) * a.Cout + n;
        float v = acc[i][j][r];
        if (a.addend) v += a.addend[at];
        if (a.relu) v = fmaxf(v, 0.0f);
        if (a.mask && !(a.mask[at] > 0.0f)) v = 0.0f;
        a.y[at] = v;
      }
    }
  }
}

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

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the workgroup's sum: per wave, then the four waves in order; valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

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
  s = block_sum_d(s, sh);
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
  if (lane == 0) sh[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

inline unsigned blocks_for(long long total) { return (unsigned)((total + kThreads - 1) / kThreads); }
constexpr long long kMaxElems = (1LL << 31) * (long long)kThreads - 1;      // one thread per element, grid.x < 2^31

int check_nhwc(const char* who, int N, int H, int W, int C) {
  DINER_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: N, H, W, C = %d, %d, %d, %d (each must be >= 1)", who, N, H, W, C);
  DINER_CHECK_ARG((long long)N * H * W <= (1LL << 40) / C, "%s: %d x %d x %d x %d elements are more than 2^40", who, N, H, W, C);
  return 0;
}

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" size_t diner_conv3x3_pack_floats(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  return (size_t)((Cin + kCK - 1) / kCK) * 9 * kCK * (size_t)((Cout + kBN - 1) / kBN * kBN);
}

extern "C" int diner_conv3x3_f32(const float* x, const float* wpack, const float* bias, const float* addend, const float* mask, float* y, int N,
                                 int H, int W, int Cin, int Cout, int relu, void* stream) {
  int rc = check_nhwc("conv3x3", N, H, W, Cin);
  if (rc) return rc;
  rc = check_nhwc("conv3x3", N, H, W, Cout);
  if (rc) return rc;
  DINER_CHECK_ARG(N <= 65535, "conv3x3: N = %d images (at most 65535 a call)", N);
  DINER_CHECK_ARG(x && wpack && y, "conv3x3: null pointer argument");
  DINER_CHECK_ARG((reinterpret_cast<uintptr_t>(wpack) & 15) == 0, "conv3x3: the packed weights are not 16-byte aligned");
  ConvArgs a;
  a.x = x; a.w = wpack; a.bias = bias; a.addend = addend; a.mask = mask; a.y = y;
  a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.CoutPad = (Cout + kBN - 1) / kBN * kBN;
  a.tiles_w = (W + kTW - 1) / kTW;
  a.relu = relu != 0;
  const long long tiles = (long long)a.tiles_w * ((H + kTH - 1) / kTH);
  DINER_CHECK_ARG(tiles < (1LL << 31) && a.CoutPad / kBN <= 65535, "conv3x3: %d x %d pixels x %d channels are too many tiles", H, W, Cout);
  hipLaunchKernelGGL(k_conv3x3, dim3((unsigned)tiles, (unsigned)(a.CoutPad / kBN), (unsigned)N), dim3(kConvThreads), 0, (hipStream_t)stream, a);
  DINER_LAUNCH_OK();
  return 0;
}

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
