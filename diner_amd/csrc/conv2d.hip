// The fp32 2-D convolution of the perceptual network (diner_amd/perceptual.py) and of the image encoder's trunk (diner_amd/encoder.py),
// activations channels-last (N,H,W,C):
//   * k_conv2d<R, S>: R x R convolution, stride S, zero padding R / 2, as an implicit GEMM on the fp32-input MFMA
//     (v_mfma_f32_16x16x4_f32, bit for bit an fmaf chain): pixels x Cout accumulators, K = R R Cin.  Built for <3,1> (the VGG stack and
//     the trunk's residual blocks), <1,2>, <3,2>, <7,2> (the trunk's downsample, first block convolution and stem) and, behind entries of
//     their own, <5,2> and <1,1> (the depth estimator's FeatureNet: its two downsampling convolutions and the 1 x 1 in front of stage 1).
//   * The accumulator starts at the bias; the epilogue adds an optional addend, applies an optional ReLU and an optional mask, and
//     writes with a channel stride and offset of the output's own (the stem writes channels 0 .. 63 of the latent directly).  With the
//     second packed weight set (taps flipped, Cin and Cout swapped) <3,1> is the data gradient: the addend is then the loss gradient
//     that enters at a tap layer, the mask the saved activation.  The weights are frozen: there is no weight gradient.
// Every output is computed in an order the shape alone fixes; a tile never crosses images (the image is blockIdx.z).
#include "common.hpp"

namespace diner {
namespace {

// A workgroup (four waves) computes an 8 x 16 tile of OUTPUT pixels of one image for 64 output channels.  One tile row = 16 pixels = the
// 16 rows of one MFMA tile, so wave w owns tile rows 2 w, 2 w + 1 (two M tiles) x four N tiles: 32 accumulator registers.  A stage is
// (chunk of 8 input channels) x (kRS kernel rows): all three rows for R = 3, ONE row for R = 7 and R = 1 -- one chunk of the stem's
// 7 x 7 x 8 x 64 weights is 100 KB, a kernel row of it 14 KB (17.5 KB with the row padding), and the input rows a kernel row touches at
// stride 2 are 8 (every second one), not 21.  Per stage the workgroup holds in LDS
//   * the input patch: kPR rows x kPC columns x 8 channels, zeros outside the image and beyond Cin (10 x 18 pixels for <3,1>: the tile
//     and a one-pixel halo).  At stride 2 the columns are split by parity into two planes, so that the 16 pixels of an operand read --
//     input columns 2 j + kx, two apart -- are neighbours in their plane and the read covers the 64 banks once, as at stride 1;
//   * the stage's kRS x R x 8 x 64 weights.
// and runs kRS x R taps x 2 k-steps x 8 MFMAs per wave between two barriers (72 for <3,1>, 112 for the stem).  Stage s + 1 travels from
// global memory into registers while stage s's MFMAs run, and moves into LDS behind the barrier that ends them: a small image gives each
// CU one workgroup, and nothing else would hide the loads.  K order of every output: chunk, kernel row, kernel column, channel -- the
// same whatever the tile or the image's place in the batch.
constexpr int kTH = 8, kTW = 16;
constexpr int kBN = DINER_CONV3X3_COUT_TILE;      // 64
constexpr int kCK = DINER_CONV3X3_CIN_CHUNK;      // 8
constexpr int kPS = kCK + 4;        // LDS words per patch pixel: 12 p + k (16 pixels x 4 k of one operand read) covers the 64 banks once
constexpr int kWS = kBN + 16;       // LDS words per weight row: the four k rows of one operand read start 16 banks apart
constexpr int kConvThreads = 256;

struct ConvArgs {
  const float* x;        // (N,H,W,Cin)
  const float* w;        // packed [ceil(Cin / 8)][ky R + kx][8][CoutPad], zeros beyond Cin and Cout
  const float* bias;     // Cout floats or null
  const float* addend;   // (N,Ho,Wo,Cout) or null: added before the ReLU and the mask (stride 1 only)
  const float* mask;     // (N,Ho,Wo,Cout) or null: the output is zero where !(mask > 0) (stride 1 only)
  float* y;              // (N,Ho,Wo,ldy), channels coff .. coff + Cout - 1
  int H, W, Cin, Cout, CoutPad, Ho, Wo, tiles_w, relu, ldy, coff;
};

template <int R, int S>
struct ConvShape {
  static constexpr int kPad = R / 2;
  static constexpr int kRS = R == 3 ? 3 : 1;                     // kernel rows per stage
  static constexpr int kStagesPerChunk = R / kRS;
  static constexpr int kPR = kRS == 1 ? kTH : S * (kTH - 1) + kRS;      // patch rows: the S-th input rows one kernel row reads, or all of them
  static constexpr int kPC = R == 1 ? kTW : S * (kTW - 1) + R;          // patch columns likewise
  static constexpr int kNQ = S == 2 && R > 1 ? 2 : 1;            // column parity planes
  static constexpr int kPCH = (kPC + kNQ - 1) / kNQ;             // columns per plane
  static constexpr int kXWords = kPR * kNQ * kPCH * kPS;
  static constexpr int kWRows = kRS * R * kCK;
  static constexpr int kWWords = kWRows * kWS;
  static constexpr int kPV = (kPR * kPC * 2 + kConvThreads - 1) / kConvThreads;        // float4 patch loads per thread
  static constexpr int kPE = (kPR * kPC * kCK + kConvThreads - 1) / kConvThreads;      // scalar patch loads per thread
  static constexpr int kWV = (kWRows * (kBN / 4) + kConvThreads - 1) / kConvThreads;   // float4 weight loads per thread
  static_assert(kNQ == 2 || S == 1 || R == 1, "one plane holds the columns of an operand read side by side only at stride 1 or R = 1");
};

template <int R, int S>
__global__ __launch_bounds__(kConvThreads) void k_conv2d(ConvArgs a) {
  using Sh = ConvShape<R, S>;
  __shared__ __attribute__((aligned(16))) float Xs[Sh::kXWords];
  __shared__ __attribute__((aligned(16))) float Ws[Sh::kWWords];
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
  const int stages = chunks * Sh::kStagesPerChunk;
  v4f xv[Sh::kPV], wv[Sh::kWV];
  float xe[Sh::kPE];
  // patch element (row r, column q) of the stage with first kernel row ky0 -> input pixel, or outside
  auto in_h = [&](int r, int ky0) { return Sh::kRS == 1 ? S * (h0 + r) + ky0 - Sh::kPad : S * h0 + r - Sh::kPad; };
  auto in_w = [&](int q) { return R == 1 ? S * (w0 + q) : S * w0 + q - Sh::kPad; };
  auto fetch = [&](int s) {
    const int c = s / Sh::kStagesPerChunk, ky0 = (s % Sh::kStagesPerChunk) * Sh::kRS, c0 = c * kCK;
    if (vec) {
#pragma unroll
      for (int u = 0; u < Sh::kPV; ++u) {
        const int e = tid + kConvThreads * u, p = e >> 1, q4 = e & 1;
        const int h = in_h(p / Sh::kPC, ky0), w = in_w(p % Sh::kPC);
        xv[u] = (v4f){0.f, 0.f, 0.f, 0.f};
        if (e < Sh::kPR * Sh::kPC * 2 && h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + 4 * q4 < a.Cin)
          xv[u] = *reinterpret_cast<const v4f*>(x + ((size_t)h * a.W + w) * a.Cin + c0 + 4 * q4);
      }
    } else {
#pragma unroll
      for (int u = 0; u < Sh::kPE; ++u) {
        const int e = tid + kConvThreads * u, p = e >> 3, k = e & 7;
        const int h = in_h(p / Sh::kPC, ky0), w = in_w(p % Sh::kPC);
        xe[u] = 0.0f;
        if (e < Sh::kPR * Sh::kPC * kCK && h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + k < a.Cin) xe[u] = x[((size_t)h * a.W + w) * a.Cin + c0 + k];
      }
    }
    const float* wsrc = a.w + ((size_t)c * R * R + (size_t)ky0 * R) * kCK * a.CoutPad + n0;
#pragma unroll
    for (int u = 0; u < Sh::kWV; ++u) {
      const int e = tid + kConvThreads * u, r = e >> 4, q = e & 15;
      if (e < Sh::kWRows * (kBN / 4)) wv[u] = *reinterpret_cast<const v4f*>(wsrc + (size_t)r * a.CoutPad + 4 * q);
    }
  };
  // LDS word of patch pixel p = row * kPC + column: with two planes the column's parity picks the plane
  auto xs_at = [&](int p) {
    if constexpr (Sh::kNQ == 1) {
      return p * kPS;
    } else {
      const int r = p / Sh::kPC, q = p % Sh::kPC;
      return ((r * 2 + (q & 1)) * Sh::kPCH + (q >> 1)) * kPS;
    }
  };
  auto stash = [&]() {
    if (vec) {
#pragma unroll
      for (int u = 0; u < Sh::kPV; ++u) {
        const int e = tid + kConvThreads * u;
        if (e < Sh::kPR * Sh::kPC * 2) *reinterpret_cast<v4f*>(&Xs[xs_at(e >> 1) + 4 * (e & 1)]) = xv[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < Sh::kPE; ++u) {
        const int e = tid + kConvThreads * u;
        if (e < Sh::kPR * Sh::kPC * kCK) Xs[xs_at(e >> 3) + (e & 7)] = xe[u];
      }
    }
#pragma unroll
    for (int u = 0; u < Sh::kWV; ++u) {
      const int e = tid + kConvThreads * u;
      if (e < Sh::kWRows * (kBN / 4)) *reinterpret_cast<v4f*>(&Ws[(e >> 4) * kWS + 4 * (e & 15)]) = wv[u];
    }
  };
  fetch(0);
  for (int s = 0; s < stages; ++s) {
    stash();
    __syncthreads();
    if (s + 1 < stages) fetch(s + 1);
#pragma unroll
    for (int t = 0; t < Sh::kRS * R; ++t) {
      const int kyl = t / R, kx = t % R;                 // kernel row within the stage, kernel column
      const int plane = Sh::kNQ == 2 ? (kx & 1) : 0, col = Sh::kNQ == 2 ? (kx >> 1) : kx;
#pragma unroll
      for (int kk = 0; kk < kCK; kk += 4) {
        float av[2], bv[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = Sh::kRS == 1 ? 2 * wave + i : S * (2 * wave + i) + kyl;
          av[i] = Xs[((row * Sh::kNQ + plane) * Sh::kPCH + lc + col) * kPS + kk + lk];
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
  const size_t img = (size_t)blockIdx.z * a.Ho * a.Wo;       // first output pixel of this image
  float* y = a.y + img * a.ldy + a.coff;
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
        const size_t pix = (size_t)h * a.Wo + w, at = (img + pix) * a.Cout + n;       // at: in the dense addend and mask
        float v = acc[i][j][r];
        if constexpr (S == 1)          // addend and mask: only stride 1 has callers for them, the stride-2 instances carry no code for them
          if (a.addend) v += a.addend[at];       // (conv2d() refuses them there): their 64 loads cost k_conv2d<1,2> a wave of occupancy
        if (a.relu) v = fmaxf(v, 0.0f);
        if constexpr (S == 1)
          if (a.mask && !(a.mask[at] > 0.0f)) v = 0.0f;
        y[pix * a.ldy + n] = v;
      }
    }
  }
}

template <int R, int S>
void launch_conv2d(const ConvArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((k_conv2d<R, S>), grid, dim3(kConvThreads), 0, stream, a);
}

size_t conv2d_pack_floats(int Cin, int Cout, int R) {
  return (size_t)((Cin + kCK - 1) / kCK) * R * R * kCK * (size_t)((Cout + kBN - 1) / kBN * kBN);
}

// the checks, the arguments and the grid of every entry; `who` begins every error text.  featurenet: the caller is one of the entries that
// reach <5,2> and <1,1>; diner_conv2d_s2_f32 keeps refusing R = 5
int conv2d(const char* who, int R, int S, const float* x, const float* wpack, const float* bias, const float* addend, const float* mask, float* y,
           int N, int H, int W, int Cin, int Cout, int relu, int ldy, int coff, hipStream_t stream, bool featurenet = false) {
  int rc = check_nhwc(who, N, H, W, Cin);
  if (rc) return rc;
  void (*launch)(const ConvArgs&, dim3, hipStream_t) = nullptr;
  if (S == 1 && R == 3) launch = launch_conv2d<3, 1>;
  else if (S == 2 && R == 1) launch = launch_conv2d<1, 2>;
  else if (S == 2 && R == 3) launch = launch_conv2d<3, 2>;
  else if (S == 2 && R == 7) launch = launch_conv2d<7, 2>;
  else if (featurenet && S == 2 && R == 5) launch = launch_conv2d<5, 2>;
  else if (featurenet && S == 1 && R == 1) launch = launch_conv2d<1, 1>;
  if (!launch) {
    set_error("%s: R = %d (the kernel sizes built are 1, 3 and 7)", who, R);
    return DINER_E_UNSUPPORTED;
  }
  DINER_CHECK_ARG(Cout >= 1, "%s: N, H, W, C = %d, %d, %d, %d (each must be >= 1)", who, N, H, W, Cout);
  DINER_CHECK_ARG(N <= 65535, "%s: N = %d images (at most 65535 a call)", who, N);
  DINER_CHECK_ARG(coff >= 0 && ldy >= 1 && Cout <= ldy - coff, "%s: channels %d .. %d do not fit an output of %d channels", who, coff,
                  coff + Cout - 1, ldy);
  const int pad = R / 2;
  const int Ho = (H + 2 * pad - R) / S + 1, Wo = (W + 2 * pad - R) / S + 1;
  rc = check_nhwc(who, N, Ho, Wo, ldy);
  if (rc) return rc;
  DINER_CHECK_ARG(x && wpack && y, "%s: null pointer argument", who);
  DINER_CHECK_ARG(S == 1 || (!addend && !mask), "%s: an addend or a mask at stride %d (the epilogue has them at stride 1 only)", who, S);
  DINER_CHECK_ARG((reinterpret_cast<uintptr_t>(wpack) & 15) == 0, "%s: the packed weights are not 16-byte aligned", who);
  ConvArgs a;
  a.x = x; a.w = wpack; a.bias = bias; a.addend = addend; a.mask = mask; a.y = y;
  a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.CoutPad = (Cout + kBN - 1) / kBN * kBN;
  a.Ho = Ho; a.Wo = Wo; a.tiles_w = (Wo + kTW - 1) / kTW;
  a.relu = relu != 0; a.ldy = ldy; a.coff = coff;
  const long long tiles = (long long)a.tiles_w * ((Ho + kTH - 1) / kTH);
  DINER_CHECK_ARG(tiles < (1LL << 31) && a.CoutPad / kBN <= 65535, "%s: %d x %d pixels x %d channels are too many tiles", who, Ho, Wo, Cout);
  launch(a, dim3((unsigned)tiles, (unsigned)(a.CoutPad / kBN), (unsigned)N), stream);
  DINER_LAUNCH_OK();
  return 0;
}

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" size_t diner_conv3x3_pack_floats(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  return conv2d_pack_floats(Cin, Cout, 3);
}

extern "C" int diner_conv3x3_f32(const float* x, const float* wpack, const float* bias, const float* addend, const float* mask, float* y, int N,
                                 int H, int W, int Cin, int Cout, int relu, void* stream) {
  return conv2d("conv3x3", 3, 1, x, wpack, bias, addend, mask, y, N, H, W, Cin, Cout, relu, Cout, 0, (hipStream_t)stream);
}

extern "C" size_t diner_conv2d_s2_pack_floats(int Cin, int Cout, int R) {
  if (Cin < 1 || Cout < 1 || (R != 1 && R != 3 && R != 7)) return 0;
  return conv2d_pack_floats(Cin, Cout, R);
}

extern "C" int diner_conv2d_s2_f32(const float* x, const float* wpack, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int R,
                                   int relu, int ldy, int coff, void* stream) {
  return conv2d("conv2d_s2", R, 2, x, wpack, bias, nullptr, nullptr, y, N, H, W, Cin, Cout, relu, ldy, coff, (hipStream_t)stream);
}

extern "C" size_t diner_conv5x5_s2_pack_floats(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  return conv2d_pack_floats(Cin, Cout, 5);
}

extern "C" int diner_conv5x5_s2_f32(const float* x, const float* wpack, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int relu,
                                    void* stream) {
  return conv2d("conv5x5_s2", 5, 2, x, wpack, bias, nullptr, nullptr, y, N, H, W, Cin, Cout, relu, Cout, 0, (hipStream_t)stream, true);
}

extern "C" size_t diner_conv1x1_pack_floats(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  return conv2d_pack_floats(Cin, Cout, 1);
}

extern "C" int diner_conv1x1_f32(const float* x, const float* wpack, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int relu,
                                 void* stream) {
  return conv2d("conv1x1", 1, 1, x, wpack, bias, nullptr, nullptr, y, N, H, W, Cin, Cout, relu, Cout, 0, (hipStream_t)stream, true);
}
