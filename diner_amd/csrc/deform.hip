// The kernels FeatureNet (the depth estimator's feature pyramid, models/module.py:343-421 of TransMVSNet) needs beyond the plain
// convolutions of conv2d.hip, activations channels-last fp32 (N,H,W,C):
//   * k_deform_conv3x3<NT, CV>: torchvision's modulated deformable convolution (deform_conv2d with a mask), 3 x 3, stride 1, padding 1,
//     dilation 1, one offset group.  offmask (N,H,W,27) is the raw output of the layer's conv_offset_mask: channel 2 k the row offset and
//     2 k + 1 the column offset of tap k = 3 ky + kx, channel 18 + k the logit of its modulation.
//       y[n,h,w,o] = bias[o] + sum_k sum_c w[o,c,ky,kx] sigmoid(offmask[18 + k]) S(x[n,:,:,c], h - 1 + ky + dy_k, w - 1 + kx + dx_k)
//     with S the bilinear sample of deform_geom.hpp.  Fused: the sampled and modulated column matrix (9 Cin numbers a pixel) lives in LDS
//     one tap at a time and never reaches global memory.
//   * k_fpn_lateral: y[n,h,w,:] = top[n,h/2,w/2,:] + (b + W lat[n,h,w,:]), the pyramid's nearest 2 x upsampling plus its 1 x 1 lateral
//     convolution with bias, one launch, no intermediate.
//
// k_deform_conv3x3.  A workgroup (four waves) computes 64 consecutive pixels (row-major) of ONE image -- blockIdx.z is the image, a tile
// never crosses images -- for 16 NT output channels (NT = 1 or 2: Cout is padded to 16 or to a multiple of 32, not to 64).  Per tap:
//   1. thread t samples pixel t >> 2: it reads the tap's two offsets and its logit, calls deform_corners() and loads, for its quarter of
//      the channels, the four corners -- each corner is one contiguous row of Cin floats of the channels-last input, read as float4 --
//      into registers (up to CV float4 a corner);
//   2. combines them as ((w00 v00 + w01 v01) + w10 v10) + w11 v11, each product and sum rounded (-ffp-contract=off), times the
//      modulation, and writes the Cin values to LDS next to the tap's Cin x 16 NT weights;
//   3. wave v multiplies pixels 16 v .. 16 v + 15 against the weights on v_mfma_f32_16x16x4_f32 (bit for bit an fmaf chain).
// The loads of tap k + 1 (step 1) are issued before the MFMAs of tap k and land in LDS behind the barrier that ends them.
// K ORDER of every output: the accumulator starts at the bias; then tap k = 0 .. 8 ascending (ky outer, kx inner), within a tap the
// input channel c = 0 .. Cin - 1 ascending.  The shape alone fixes it: no atomics, no split K, the same bits at any batch position.
// A corner that deform_corners() does not mark valid is never addressed; a pixel beyond the image's last is neither sampled nor written.
#include "common.hpp"
#include "deform_geom.hpp"

namespace diner {
namespace {

constexpr int kDfPix = 64;                          // output pixels a workgroup: four waves x the 16 rows of one MFMA tile
constexpr int kDfThreads = 256;
constexpr int kDfMaxCin = DINER_DEFORM_MAX_CIN;     // 64
constexpr int kDfTaps = 9;

struct DeformArgs {
  const float* x;        // (N,H,W,Cin)
  const float* om;       // (N,H,W,27)
  const float* w;        // packed [ceil(Cout / BN)][tap][Cin][BN], BN = 16 NT, zeros beyond Cout
  const float* bias;     // Cout floats or null
  float* y;              // (N,H,W,Cout)
  int H, W, Cin, Cout, relu;
};

template <int NT, int CV>
__global__ __launch_bounds__(kDfThreads) void k_deform_conv3x3(DeformArgs a) {
  constexpr int BN = 16 * NT;
  constexpr int WS = NT == 1 ? 16 : 48;       // LDS words a weight row: the four k rows of one operand read start 16 banks apart
  constexpr int WV = (kDfMaxCin * BN / 4 + kDfThreads - 1) / kDfThreads;       // float4 weight loads a thread and tap
  __shared__ __attribute__((aligned(16))) float Cs[kDfPix * (kDfMaxCin + 4)];
  __shared__ __attribute__((aligned(16))) float Ws[kDfMaxCin * WS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
  const int HW = a.H * a.W, Cin = a.Cin;
  const int XS = Cin + 4;                     // words a pixel's row of Cs: (Cin / 4 + 1) is odd, so 16 pixels x 4 k cover the 64 banks once
  const int p0 = (int)blockIdx.x * kDfPix, n0 = (int)blockIdx.y * BN;
  const size_t img = blockIdx.z;
  const float* x = a.x + img * HW * Cin;
  const float* om = a.om + img * HW * 27;
  // the sampling role: pixel sp, channel float4s sq, sq + 4, ...
  const int sp = tid >> 2, sq = tid & 3, spix = p0 + sp;
  const bool live = spix < HW;
  const int sh = live ? spix / a.W : 0, sw = live ? spix % a.W : 0;
  const int c4n = Cin >> 2;

  v4f acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + 16 * j + lc;
    const float b = (a.bias && n < a.Cout) ? a.bias[n] : 0.0f;          // D layout: column lane & 15 in all four registers
    acc[j] = (v4f){b, b, b, b};
  }

  v4f cv[CV][4], wv[WV];
  float cw[4], cm;
  auto fetch = [&](int k) {
    DeformCorners c = deform_corners(0, 0, 0, 0, -2.0f, -2.0f, 1, 1);           // outside: nothing valid
    cm = 0.0f;
    if (live) {
      const float* o = om + (size_t)spix * 27;
      c = deform_corners(sh, sw, k / 3, k % 3, o[2 * k], o[2 * k + 1], a.H, a.W);
      cm = 1.0f / (1.0f + expf(-o[18 + k]));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cw[i] = c.wt[i];
#pragma unroll
    for (int u = 0; u < CV; ++u) {
      const int c4 = sq + 4 * u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cv[u][i] = (v4f){0.f, 0.f, 0.f, 0.f};
        if (((c.valid >> i) & 1u) && c4 < c4n) cv[u][i] = *reinterpret_cast<const v4f*>(x + (size_t)c.idx[i] * Cin + 4 * c4);
      }
    }
    const float* wsrc = a.w + ((size_t)blockIdx.y * kDfTaps + k) * Cin * BN;
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int e = tid + kDfThreads * u;
      if (e < Cin * (BN / 4)) wv[u] = *reinterpret_cast<const v4f*>(wsrc + 4 * e);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < CV; ++u) {
      const int c4 = sq + 4 * u;
      if (c4 < c4n) {
        const v4f v = ((cw[0] * cv[u][0] + cw[1] * cv[u][1]) + cw[2] * cv[u][2]) + cw[3] * cv[u][3];
        *reinterpret_cast<v4f*>(&Cs[sp * XS + 4 * c4]) = v * cm;
      }
    }
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int e = tid + kDfThreads * u;
      if (e < Cin * (BN / 4)) *reinterpret_cast<v4f*>(&Ws[(e / (BN / 4)) * WS + 4 * (e % (BN / 4))]) = wv[u];
    }
  };

  fetch(0);
  for (int k = 0; k < kDfTaps; ++k) {
    stash();
    __syncthreads();
    if (k + 1 < kDfTaps) fetch(k + 1);
    const float* arow = &Cs[(16 * wave + lc) * XS + lk];
    for (int kk = 0; kk < Cin; kk += 4) {
      const float av = arow[kk];
      float bv[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) bv[j] = Ws[(kk + lk) * WS + 16 * j + lc];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }

  // D layout: lane holds rows (pixels) 4 (lane >> 4) .. + 3 of column (output channel) lane & 15
  float* y = a.y + img * HW * a.Cout;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + 16 * j + lc;
    if (n >= a.Cout) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = p0 + 16 * wave + 4 * lk + r;
      if (p >= HW) continue;
      float v = acc[j][r];
      if (a.relu) v = fmaxf(v, 0.0f);
      y[(size_t)p * a.Cout + n] = v;
    }
  }
}

template <int NT, int CV>
void launch_deform(const DeformArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((k_deform_conv3x3<NT, CV>), grid, dim3(kDfThreads), 0, stream, a);
}

int deform_bn(int Cout) { return Cout <= 16 ? 16 : 32; }

// ---- the pyramid's lateral ----------------------------------------------------------------------------------------------------------------
constexpr int kLatMaxC = DINER_FPN_MAX_CHANNELS;   // 64

// one thread: four output channels of one fine pixel; each a chain that starts at the bias, k ascending, then + the coarse pixel
__global__ __launch_bounds__(256) void k_fpn_lateral(const float* __restrict__ top, const float* __restrict__ lat, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ y, long long total, int H, int W,
                                                      int Ctop, int Clat) {
  __shared__ __attribute__((aligned(16))) float Wt[kLatMaxC * kLatMaxC];        // [k][co]: a thread reads four neighbours of one k
  for (int e = threadIdx.x; e < Ctop * Clat; e += 256) Wt[(e % Clat) * Ctop + e / Clat] = w[e];         // w is (Ctop, Clat) row-major
  __syncthreads();
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int quads = Ctop / 4, q = (int)(e % quads);
  const long long pix = e / quads;
  const int ox = (int)(pix % W), oy = (int)((pix / W) % H);
  const long long n = pix / ((long long)W * H);
  const float* l = lat + pix * Clat;
  v4f acc = bias ? (v4f){bias[4 * q], bias[4 * q + 1], bias[4 * q + 2], bias[4 * q + 3]} : (v4f){0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < Clat; ++k) {
    const float lv = l[k];
    const v4f wk = *reinterpret_cast<const v4f*>(&Wt[k * Ctop + 4 * q]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaf(lv, wk[j], acc[j]);
  }
  const v4f t = *reinterpret_cast<const v4f*>(top + ((n * (H / 2) + oy / 2) * (W / 2) + ox / 2) * Ctop + 4 * q);
  *reinterpret_cast<v4f*>(y + 4 * e) = t + acc;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" size_t diner_deform_conv3x3_pack_floats(int Cin, int Cout) {
  if (Cin < 8 || Cin > kDfMaxCin || Cin % 8 != 0 || Cout < 1) return 0;
  const int bn = deform_bn(Cout);
  return (size_t)((Cout + bn - 1) / bn) * kDfTaps * Cin * bn;
}

extern "C" int diner_deform_conv3x3_f32(const float* x, const float* offmask, const float* wpack, const float* bias, float* y, int N, int H, int W,
                                        int Cin, int Cout, int relu, void* stream) {
  int rc = check_nhwc("deform_conv3x3", N, H, W, Cin);
  if (rc) return rc;
  DINER_CHECK_ARG(Cin >= 8 && Cin <= kDfMaxCin && Cin % 8 == 0, "deform_conv3x3: Cin = %d (a multiple of 8 in [8, %d])", Cin, kDfMaxCin);
  DINER_CHECK_ARG(Cout >= 1, "deform_conv3x3: Cout = %d (must be >= 1)", Cout);
  DINER_CHECK_ARG(N <= 65535, "deform_conv3x3: N = %d images (at most 65535 a call)", N);
  DINER_CHECK_ARG(H <= (1 << 14) && W <= (1 << 14), "deform_conv3x3: H, W = %d, %d (each at most 2^14)", H, W);
  rc = check_nhwc("deform_conv3x3", N, H, W, Cout);
  if (rc) return rc;
  DINER_CHECK_ARG(x && offmask && wpack && y, "deform_conv3x3: null pointer argument");
  DINER_CHECK_ARG(y != x && y != offmask, "deform_conv3x3: y must not be one of the inputs (other tiles still read them)");
  DINER_CHECK_ARG(aligned16(x) && aligned16(wpack), "deform_conv3x3: x and the packed weights must be 16-byte aligned");
  DINER_CHECK_ARG((reinterpret_cast<uintptr_t>(offmask) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(bias) & 3) == 0,
                  "deform_conv3x3: offmask, bias and y must be 4-byte aligned");
  const int bn = deform_bn(Cout), ntiles = (Cout + bn - 1) / bn;
  DINER_CHECK_ARG(ntiles <= 65535, "deform_conv3x3: Cout = %d output channels are too many column tiles", Cout);
  DeformArgs a;
  a.x = x; a.om = offmask; a.w = wpack; a.bias = bias; a.y = y;
  a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.relu = relu != 0;
  const dim3 grid((unsigned)((H * W + kDfPix - 1) / kDfPix), (unsigned)ntiles, (unsigned)N);
  const int cv = Cin <= 16 ? 1 : Cin <= 32 ? 2 : 4;
  void (*launch)(const DeformArgs&, dim3, hipStream_t) =
      bn == 16 ? (cv == 1 ? launch_deform<1, 1> : cv == 2 ? launch_deform<1, 2> : launch_deform<1, 4>)
               : (cv == 1 ? launch_deform<2, 1> : cv == 2 ? launch_deform<2, 2> : launch_deform<2, 4>);
  launch(a, grid, (hipStream_t)stream);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_fpn_lateral_f32(const float* top, const float* lateral, const float* w, const float* bias, float* y, int N, int H, int W,
                                     int Ctop, int Clat, void* stream) {
  int rc = check_nhwc("fpn_lateral", N, H, W, Clat);
  if (rc) return rc;
  DINER_CHECK_ARG(H % 2 == 0 && W % 2 == 0 && H <= (1 << 15) && W <= (1 << 15), "fpn_lateral: H, W = %d, %d (the fine size: even, at most 2^15)", H, W);
  DINER_CHECK_ARG(Ctop >= 4 && Ctop <= kLatMaxC && Ctop % 4 == 0 && Clat <= kLatMaxC,
                  "fpn_lateral: Ctop = %d, Clat = %d (Ctop a multiple of 4 in [4, %d], Clat at most %d)", Ctop, Clat, kLatMaxC, kLatMaxC);
  rc = check_nhwc("fpn_lateral", N, H, W, Ctop);
  if (rc) return rc;
  const long long total = (long long)N * H * W * (Ctop / 4);
  DINER_CHECK_ARG((total + 255) / 256 < (1LL << 31), "fpn_lateral: %d x %d x %d x %d outputs are too many for one launch", N, H, W, Ctop);
  DINER_CHECK_ARG(top && lateral && w && y, "fpn_lateral: null pointer argument");
  DINER_CHECK_ARG(aligned16(top) && aligned16(y), "fpn_lateral: top and y must be 16-byte aligned");
  DINER_CHECK_ARG(y != top && y != lateral, "fpn_lateral: y must not be one of the inputs");
  hipLaunchKernelGGL(k_fpn_lateral, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, top, lateral, w, bias, y, total, H, W,
                     Ctop, Clat);
  DINER_LAUNCH_OK();
  return 0;
}
