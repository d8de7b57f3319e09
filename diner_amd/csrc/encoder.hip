// The image encoder's trunk on the device (diner_amd/encoder.py): what SpatialEncoder.forward (image_encoder.py of the reference, :225-291)
// needs beside the stride-1 3 x 3 convolution of perceptual.hip, all fp32, activations channels-last (N,H,W,C):
//   * k_conv_s2<R>: R x R convolution (R = 1, 3, 7), stride 2, zero padding R / 2, as an implicit GEMM on the fp32-input MFMA
//     (v_mfma_f32_16x16x4_f32, bit for bit an fmaf chain): pixels x Cout accumulators, K = R R Cin; epilogue + bias (the accumulator
//     starts there) and an optional ReLU; the output has a channel stride and offset of its own, so the stem writes channels 0 .. 63 of
//     the latent directly.
//   * k_maxpool3s2: MaxPool2d(3, 2, 1); the input has a channel stride (it reads the stem's output inside the latent).
//   * k_encoder_input: (N,3,H,W) -> channels-last, replication-padded, with the positional-encoding ring channels and zero channels
//     behind them (the stem reads 24 channels, not 21: float4 loads).
//   * k_pyramid_level: bilinear align_corners=True resampling of one pyramid level into its channel slice of the latent.
// Every output is computed in an order the shape alone fixes; a tile never crosses images (the image is blockIdx.z).
#include <cmath>
#include "common.hpp"

namespace diner {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

// ---- the strided convolution -----------------------------------------------------------------------------------------------------------
// The tiling of k_conv3x3 (perceptual.hip): a workgroup (four waves) computes an 8 x 16 tile of OUTPUT pixels of one image for 64 output
// channels; one tile row = the 16 rows of one MFMA tile, wave w owns tile rows 2 w, 2 w + 1 (two M tiles) x four N tiles = 32 accumulator
// registers.  What differs is the staging.  A stage is (chunk of 8 input channels) x (kRS kernel rows): all three rows for R = 3, ONE row
// for R = 7 and R = 1 -- one chunk of the stem's 7 x 7 x 8 x 64 weights is 100 KB, a kernel row of it 14 KB (17.5 KB with the row
// padding), and the input rows a kernel row touches are 8 (every second one), not 21.  Per stage the workgroup holds in LDS
//   * the input patch: kPR rows x kPC columns x 8 channels (12 words a pixel, as in k_conv3x3), zeros outside the image and beyond Cin.
//     Columns are split by parity into two planes, so that the 16 pixels of an operand read -- input columns 2 j + kx, two apart -- are
//     neighbours in their plane and the read covers the 64 banks once, as at stride 1;
//   * the stage's kRS x R x 8 x 64 weights (80 words a row).
// and runs kRS x R taps x 2 k-steps x 8 MFMAs per wave between two barriers (112 for the stem) while the next stage's loads are in
// flight in registers.  K order of every output: chunk, kernel row, kernel column, channel.
constexpr int kTH = 8, kTW = 16;
constexpr int kBN = DINER_CONV3X3_COUT_TILE;      // 64
constexpr int kCK = DINER_CONV3X3_CIN_CHUNK;      // 8
constexpr int kPS = kCK + 4;
constexpr int kWS = kBN + 16;
constexpr int kConvThreads = 256;

struct ConvS2Args {
  const float* x;        // (N,H,W,Cin)
  const float* w;        // packed [ceil(Cin / 8)][R R][8][CoutPad], zeros beyond Cin and Cout
  const float* bias;     // Cout floats or null
  float* y;              // (N,Ho,Wo,ldy), channels coff .. coff + Cout - 1
  int H, W, Cin, Cout, CoutPad, Ho, Wo, tiles_w, relu, ldy, coff;
};

template <int R>
struct ConvS2Shape {
  static constexpr int kPad = R / 2;
  static constexpr int kRS = R == 3 ? 3 : 1;                     // kernel rows per stage
  static constexpr int kStagesPerChunk = R / kRS;
  static constexpr int kPR = kRS == 1 ? kTH : 2 * (kTH - 1) + kRS;      // patch rows: every second input row, or all of them
  static constexpr int kPC = R == 1 ? kTW : 2 * (kTW - 1) + R;          // patch columns likewise
  static constexpr int kNQ = R == 1 ? 1 : 2;                     // column parity planes
  static constexpr int kPCH = (kPC + kNQ - 1) / kNQ;             // columns per plane
  static constexpr int kXWords = kPR * kNQ * kPCH * kPS;
  static constexpr int kWRows = kRS * R * kCK;
  static constexpr int kWWords = kWRows * kWS;
  static constexpr int kPV = (kPR * kPC * 2 + kConvThreads - 1) / kConvThreads;        // float4 patch loads per thread
  static constexpr int kPE = (kPR * kPC * kCK + kConvThreads - 1) / kConvThreads;      // scalar patch loads per thread
  static constexpr int kWV = (kWRows * (kBN / 4) + kConvThreads - 1) / kConvThreads;   // float4 weight loads per thread
};

template <int R>
__global__ __launch_bounds__(kConvThreads) void k_conv_s2(ConvS2Args a) {
  using S = ConvS2Shape<R>;
  __shared__ __attribute__((aligned(16))) float Xs[S::kXWords];
  __shared__ __attribute__((aligned(16))) float Ws[S::kWWords];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = ((int)blockIdx.x / a.tiles_w) * kTH, w0 = ((int)blockIdx.x % a.tiles_w) * kTW, n0 = (int)blockIdx.y * kBN;
  const float* x = a.x + (size_t)blockIdx.z * a.H * a.W * a.Cin;       // this image: a tile never leaves it
  const int lc = lane & 15, lk = lane >> 4;
  v4f acc[2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + 16 * j + lc;
    const float b = (a.bias && n < a.Cout) ? a.bias[n] : 0.0f;          // D layout: column lane & 15 in all four registers
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i][j] = (v4f){b, b, b, b};
  }
  const bool vec = (a.Cin & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  const int chunks = (a.Cin + kCK - 1) / kCK;
  const int stages = chunks * S::kStagesPerChunk;
  v4f xv[S::kPV], wv[S::kWV];
  float xe[S::kPE];
  // patch element (row r, column q) of the stage with first kernel row ky0 -> input pixel, or outside
  auto in_h = [&](int r, int ky0) { return S::kRS == 1 ? 2 * (h0 + r) + ky0 - S::kPad : 2 * h0 + r - S::kPad; };
  auto in_w = [&](int q) { return R == 1 ? 2 * (w0 + q) : 2 * w0 + q - S::kPad; };
  auto fetch = [&](int s) {
    const int c = s / S::kStagesPerChunk, ky0 = (s % S::kStagesPerChunk) * S::kRS, c0 = c * kCK;
    if (vec) {
#pragma unroll
      for (int u = 0; u < S::kPV; ++u) {
        const int e = tid + kConvThreads * u, p = e >> 1, q4 = e & 1;
        const int h = in_h(p / S::kPC, ky0), w = in_w(p % S::kPC);
        xv[u] = (v4f){0.f, 0.f, 0.f, 0.f};
        if (e < S::kPR * S::kPC * 2 && h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + 4 * q4 < a.Cin)
          xv[u] = *reinterpret_cast<const v4f*>(x + ((size_t)h * a.W + w) * a.Cin + c0 + 4 * q4);
      }
    } else {
#pragma unroll
      for (int u = 0; u < S::kPE; ++u) {
        const int e = tid + kConvThreads * u, p = e >> 3, k = e & 7;
        const int h = in_h(p / S::kPC, ky0), w = in_w(p % S::kPC);
        xe[u] = 0.0f;
        if (e < S::kPR * S::kPC * kCK && h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + k < a.Cin) xe[u] = x[((size_t)h * a.W + w) * a.Cin + c0 + k];
      }
    }
    const float* wsrc = a.w + ((size_t)c * R * R + (size_t)ky0 * R) * kCK * a.CoutPad + n0;
#pragma unroll
    for (int u = 0; u < S::kWV; ++u) {
      const int e = tid + kConvThreads * u, r = e >> 4, q = e & 15;
      if (e < S::kWRows * (kBN / 4)) wv[u] = *reinterpret_cast<const v4f*>(wsrc + (size_t)r * a.CoutPad + 4 * q);
    }
  };
  // LDS word of patch pixel p = row * kPC + column: the column's parity picks the plane
  auto xs_at = [&](int p) {
    const int r = p / S::kPC, q = p % S::kPC;
    return ((r * S::kNQ + (S::kNQ == 2 ? (q & 1) : 0)) * S::kPCH + (S::kNQ == 2 ? (q >> 1) : q)) * kPS;
  };
  auto stash = [&]() {
    if (vec) {
#pragma unroll
      for (int u = 0; u < S::kPV; ++u) {
        const int e = tid + kConvThreads * u;
        if (e < S::kPR * S::kPC * 2) *reinterpret_cast<v4f*>(&Xs[xs_at(e >> 1) + 4 * (e & 1)]) = xv[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < S::kPE; ++u) {
        const int e = tid + kConvThreads * u;
        if (e < S::kPR * S::kPC * kCK) Xs[xs_at(e >> 3) + (e & 7)] = xe[u];
      }
    }
#pragma unroll
    for (int u = 0; u < S::kWV; ++u) {
      const int e = tid + kConvThreads * u;
      if (e < S::kWRows * (kBN / 4)) *reinterpret_cast<v4f*>(&Ws[(e >> 4) * kWS + 4 * (e & 15)]) = wv[u];
    }
  };
  fetch(0);
  for (int s = 0; s < stages; ++s) {
    stash();
    __syncthreads();
    if (s + 1 < stages) fetch(s + 1);
#pragma unroll
    for (int t = 0; t < S::kRS * R; ++t) {
      const int kyl = t / R, kx = t % R;                 // kernel row within the stage, kernel column
      const int plane = S::kNQ == 2 ? (kx & 1) : 0, col = S::kNQ == 2 ? (kx >> 1) : 0;
#pragma unroll
      for (int kk = 0; kk < kCK; kk += 4) {
        float av[2], bv[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = S::kRS == 1 ? 2 * wave + i : 2 * (2 * wave + i) + kyl;
          av[i] = Xs[((row * S::kNQ + plane) * S::kPCH + lc + col) * kPS + kk + lk];
        }
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
  float* y = a.y + (size_t)blockIdx.z * a.Ho * a.Wo * a.ldy + a.coff;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int h = h0 + 2 * wave + i;
    if (h >= a.Ho) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + 16 * j + lc;
      if (n >= a.Cout) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int w = w0 + 4 * lk + r;
        if (w >= a.Wo) continue;
        float v = acc[i][j][r];
        if (a.relu) v = fmaxf(v, 0.0f);
        y[((size_t)h * a.Wo + w) * a.ldy + n] = v;
      }
    }
  }
}

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

int check_nhwc(const char* who, int N, int H, int W, int C) {
  DINER_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: N, H, W, C = %d, %d, %d, %d (each must be >= 1)", who, N, H, W, C);
  DINER_CHECK_ARG((long long)N * H * W <= (1LL << 40) / C, "%s: %d x %d x %d x %d elements are more than 2^40", who, N, H, W, C);
  return 0;
}

template <int R>
void launch_conv_s2(const ConvS2Args& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(k_conv_s2<R>, grid, dim3(kConvThreads), 0, stream, a);
}

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" size_t diner_conv2d_s2_pack_floats(int Cin, int Cout, int R) {
  if (Cin < 1 || Cout < 1 || (R != 1 && R != 3 && R != 7)) return 0;
  return (size_t)((Cin + kCK - 1) / kCK) * R * R * kCK * (size_t)((Cout + kBN - 1) / kBN * kBN);
}

extern "C" int diner_conv2d_s2_f32(const float* x, const float* wpack, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int R,
                                   int relu, int ldy, int coff, void* stream) {
  int rc = check_nhwc("conv2d_s2", N, H, W, Cin);
  if (rc) return rc;
  if (R != 1 && R != 3 && R != 7) {
    set_error("conv2d_s2: R = %d (the kernel sizes built are 1, 3 and 7)", R);
    return DINER_E_UNSUPPORTED;
  }
  DINER_CHECK_ARG(Cout >= 1, "conv2d_s2: N, H, W, C = %d, %d, %d, %d (each must be >= 1)", N, H, W, Cout);
  DINER_CHECK_ARG(N <= 65535, "conv2d_s2: N = %d images (at most 65535 a call)", N);
  DINER_CHECK_ARG(coff >= 0 && ldy >= 1 && Cout <= ldy - coff, "conv2d_s2: channels %d .. %d do not fit an output of %d channels", coff,
                  coff + Cout - 1, ldy);
  const int pad = R / 2;
  const int Ho = (H + 2 * pad - R) / 2 + 1, Wo = (W + 2 * pad - R) / 2 + 1;
  rc = check_nhwc("conv2d_s2", N, Ho, Wo, ldy);
  if (rc) return rc;
  DINER_CHECK_ARG(x && wpack && y, "conv2d_s2: null pointer argument");
  DINER_CHECK_ARG((reinterpret_cast<uintptr_t>(wpack) & 15) == 0, "conv2d_s2: the packed weights are not 16-byte aligned");
  ConvS2Args a;
  a.x = x; a.w = wpack; a.bias = bias; a.y = y;
  a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.CoutPad = (Cout + kBN - 1) / kBN * kBN;
  a.Ho = Ho; a.Wo = Wo; a.tiles_w = (Wo + kTW - 1) / kTW;
  a.relu = relu != 0; a.ldy = ldy; a.coff = coff;
  const long long tiles = (long long)a.tiles_w * ((Ho + kTH - 1) / kTH);
  DINER_CHECK_ARG(tiles < (1LL << 31) && a.CoutPad / kBN <= 65535, "conv2d_s2: %d x %d pixels x %d channels are too many tiles", Ho, Wo, Cout);
  const dim3 grid((unsigned)tiles, (unsigned)(a.CoutPad / kBN), (unsigned)N);
  if (R == 1) launch_conv_s2<1>(a, grid, (hipStream_t)stream);
  else if (R == 3) launch_conv_s2<3>(a, grid, (hipStream_t)stream);
  else launch_conv_s2<7>(a, grid, (hipStream_t)stream);
  DINER_LAUNCH_OK();
  return 0;
}

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
