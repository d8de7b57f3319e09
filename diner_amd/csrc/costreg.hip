// The depth estimator's cost regulariser on the device (diner_amd/mvs.py, DeviceCostRegNet): the two layer kinds of TransMVSNet's
// CostRegNet (models/module.py:424-455), a 3-D U-Net of eleven 3 x 3 x 3 layers, all fp32, activations channels-last (N,D,H,W,C):
//   * k_conv3d<STRIDE, NT>: 3 x 3 x 3 convolution, stride 1 or 2, zero padding 1, as an implicit GEMM on the fp32-input MFMA
//     (v_mfma_f32_16x16x4_f32, bit for bit an fmaf chain): output voxels x Cout accumulators, K = 27 Cin.
//   * k_deconv3d_s2<NT>: ConvTranspose3d(3, stride 2, padding 1, output_padding 1) as a GATHER: output index o receives input i through
//     tap k = o + 1 - 2 i, so an even o has one tap (k = 1, i = o / 2) and an odd o two (k = 0 at i = (o + 1) / 2, k = 2 at
//     i = (o - 1) / 2; i = n_in contributes zero).  The eight parity classes of (od, oh, ow) have 1, 2, 2, 2, 4, 4, 4, 8 taps; a workgroup
//     computes ONE class, so its tap set is uniform and every MFMA is a needed one.  No scatter, no atomics.
// Both share one body.  Epilogue: ReLU if asked, THEN + addend (the U-Net adds its skip tensors after the activation:
// x = conv4 + relu(bn(deconv(x)))) -- the other order than k_conv2d's (conv2d.hip).  The accumulator starts at the bias and takes one sum
// per channel chunk, each chunk's sum an fmaf chain from zero (this keeps the rounding error of Cin 64 near that of Cin 8); K order of
// every output: channel chunk of 8, then kd, kh, kw ascending (the taps a class has, for the transposed layer), then channel -- fixed by
// the shape alone.  A workgroup never crosses samples (blockIdx.z is the sample), so a sample's bits do not depend on its batch position.
// The N tile is 16 wide; a workgroup runs NT = 1, 2 or 4 of them (Cout <= 16, <= 32, more), so Cout = 8 wastes half an MFMA tile, not 7/8.
// conv0 (Cin 1) and prob (Cout 1) are bandwidth-bound and run on two plain VALU kernels with the same K order (k_conv3d_cin1 /
// k_conv3d_cout1, below); any other thin shape (stride 2, Cin 1 with Cout > 16, Cout 1 with Cin not 4 or 8) takes the MFMA kernels.
#include <cstdint>
#include "common.hpp"

namespace diner {
namespace {

constexpr int kCK = DINER_CONV3D_CIN_CHUNK;       // 8
constexpr int kNT = DINER_CONV3D_COUT_TILE;       // 16
constexpr int kPS = kCK + 4;        // LDS words per patch voxel: 12 p + k (16 voxels x 4 k of one operand read) covers the 64 banks once
constexpr int kTW = 16;             // one tile row along W = the 16 rows of one MFMA tile
constexpr int kThreads = 256;
constexpr int kFillWorkgroups = 1024;   // four workgroups for each of the 256 compute units
constexpr int kStepTaps = 9;       // weights are staged for at most nine taps at a time (one kd of a convolution; a whole parity class)

enum { kConvS1 = 0, kConvS2 = 1, kDeconv = 2 };

// A workgroup (four waves) computes TD x TH x 16 output voxels (for the transposed layer: that many voxels of one parity class, a tile of
// the INPUT grid) for 16 NT output channels; wave w owns MI = TD TH / 4 tile rows.  Patch: the input voxels those outputs read.
template <int MODE> struct Tile;
template <> struct Tile<kConvS1> { static constexpr int TD = 2, TH = 4, S = 1, PD = 4, PH = 6, PW = 18; };
// stride 2: the patch's columns are stored split by parity (even columns first), so that the 16 voxels of one operand read -- columns
// 2 lc + kw -- lie 12 words apart like stride 1's and cover the banks once (as k_conv2d does at stride 2, conv2d.hip)
template <> struct Tile<kConvS2> { static constexpr int TD = 2, TH = 2, S = 2, PD = 5, PH = 5, PW = 33; };
// transposed: a class reads input voxels q and q + 1 per axis, at unit stride; its STORES are what is strided (every other voxel per axis)
template <> struct Tile<kDeconv> { static constexpr int TD = 2, TH = 4, S = 1, PD = 3, PH = 5, PW = 17; };

struct Conv3dArgs {
  const float* x;        // (N,D,H,W,Cin)
  const float* w;        // packed [ceil(Cin / 8)][27][8][CoutPad], zeros beyond Cin and Cout
  const float* bias;     // Cout floats or null
  const float* addend;   // (N,Do,Ho,Wo,Cout) or null: added after the ReLU
  float* y;              // (N,Do,Ho,Wo,Cout)
  int D, H, W, Do, Ho, Wo, Cin, Cout, CoutPad, tiles_h, tiles_w, relu;
};

template <int NT> constexpr int weight_stride() { return NT == 1 ? 16 : 16 * NT + 16; }    // the four k rows of one operand read start 16 banks apart

// the transposed layer's tap t of class (pd, ph, pw), taps in ascending (kd, kh, kw) order: per axis parity 0 has k = 1 at offset 0;
// parity 1 has k = 0 at input offset + 1, then k = 2 at offset 0
__device__ __forceinline__ void deconv_tap(int t, int pd, int ph, int pw, int* tap, int* od, int* oh, int* ow) {
  const int iw = t & pw, t2 = t >> pw, ih = t2 & ph, id = (t2 >> ph) & pd;
  const int kd = pd ? 2 * id : 1, kh = ph ? 2 * ih : 1, kw = pw ? 2 * iw : 1;
  *od = pd ? 1 - id : 0;
  *oh = ph ? 1 - ih : 0;
  *ow = pw ? 1 - iw : 0;
  *tap = (kd * 3 + kh) * 3 + kw;
}

template <int MODE, int NT>
__device__ __forceinline__ void conv3d_body(const Conv3dArgs& a, float* Xs, float* Ws) {
  using T = Tile<MODE>;
  constexpr int TD = T::TD, TH = T::TH, S = T::S, PD = T::PD, PH = T::PH, PW = T::PW;
  constexpr int MI = TD * TH / 4;
  constexpr int WS = weight_stride<NT>();
  constexpr int kEven = (PW + 1) / 2;                       // stride 2: slots of the even patch columns
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lk = lane >> 4;
  int bx = (int)blockIdx.x, cls = 0;
  if (MODE == kDeconv) { cls = bx & 7; bx >>= 3; }
  const int pd = cls >> 2, ph = (cls >> 1) & 1, pw = cls & 1;
  const int w0 = (bx % a.tiles_w) * kTW;
  bx /= a.tiles_w;
  const int h0 = (bx % a.tiles_h) * TH, d0 = (bx / a.tiles_h) * TD;
  const int n0 = (int)blockIdx.y * 16 * NT;
  const float* x = a.x + (size_t)blockIdx.z * a.D * a.H * a.W * a.Cin;       // this sample: a tile never leaves it
  const int gd0 = MODE == kDeconv ? d0 : d0 * S - 1, gh0 = MODE == kDeconv ? h0 : h0 * S - 1, gw0 = MODE == kDeconv ? w0 : w0 * S - 1;

  v4f acc[MI][NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + 16 * j + lc;
    const float b = (a.bias && n < a.Cout) ? a.bias[n] : 0.0f;          // D layout: column lane & 15 in all four registers
#pragma unroll
    for (int i = 0; i < MI; ++i) acc[i][j] = (v4f){b, b, b, b};
  }
  const bool vec = (a.Cin & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  const int chunks = (a.Cin + kCK - 1) / kCK;
  const int steps = MODE == kDeconv ? 1 : 3;                               // weight stagings per chunk: one per kd; one per class
  const int step_taps = MODE == kDeconv ? (1 << (pd + ph + pw)) : kStepTaps;

  for (int c = 0; c < chunks; ++c) {
    const int c0 = c * kCK;
    // the chunk's 27 x 8 products form a chain of their own from zero; the chunk sums then join the accumulator in chunk order: at
    // Cin 64 one chain of 1728 terms would carry about three times the rounding error of eight chains of 216
    v4f part[MI][NT];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) part[i][j] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < steps; ++s) {
      __syncthreads();                                                     // the previous step's operand reads are done
      if (s == 0) {
        if (vec) {
          for (int e = tid; e < PD * PH * PW * 2; e += kThreads) {
            const int p = e >> 1, q = e & 1;
            const int px = p % PW, py = (p / PW) % PH, pz = p / (PW * PH);
            const int d = gd0 + pz, h = gh0 + py, w = gw0 + px;
            v4f v = (v4f){0.f, 0.f, 0.f, 0.f};
            if (d >= 0 && d < a.D && h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + 4 * q < a.Cin)
              v = *reinterpret_cast<const v4f*>(x + (((size_t)d * a.H + h) * a.W + w) * a.Cin + c0 + 4 * q);
            const int slot = MODE == kConvS2 ? (px & 1) * kEven + (px >> 1) : px;
            *reinterpret_cast<v4f*>(&Xs[((pz * PH + py) * PW + slot) * kPS + 4 * q]) = v;
          }
        } else {
          for (int e = tid; e < PD * PH * PW * kCK; e += kThreads) {
            const int p = e >> 3, k = e & 7;
            const int px = p % PW, py = (p / PW) % PH, pz = p / (PW * PH);
            const int d = gd0 + pz, h = gh0 + py, w = gw0 + px;
            float v = 0.0f;
            if (d >= 0 && d < a.D && h >= 0 && h < a.H && w >= 0 && w < a.W && c0 + k < a.Cin)
              v = x[(((size_t)d * a.H + h) * a.W + w) * a.Cin + c0 + k];
            const int slot = MODE == kConvS2 ? (px & 1) * kEven + (px >> 1) : px;
            Xs[((pz * PH + py) * PW + slot) * kPS + k] = v;
          }
        }
      }
      // this step's weights: step_taps x 8 rows of 16 NT floats
      for (int e = tid; e < step_taps * kCK * 4 * NT; e += kThreads) {
        const int r = e / (4 * NT), q = e % (4 * NT);
        int tap = s * kStepTaps + (r >> 3), od, oh, ow;
        if (MODE == kDeconv) deconv_tap(r >> 3, pd, ph, pw, &tap, &od, &oh, &ow);
        *reinterpret_cast<v4f*>(&Ws[r * WS + 4 * q]) =
            *reinterpret_cast<const v4f*>(a.w + (((size_t)c * 27 + tap) * kCK + (r & 7)) * a.CoutPad + n0 + 4 * q);
      }
      __syncthreads();
      if (MODE == kDeconv) {
        for (int t = 0; t < step_taps; ++t) {
          int tap, od, oh, ow;
          deconv_tap(t, pd, ph, pw, &tap, &od, &oh, &ow);
#pragma unroll
          for (int kk = 0; kk < kCK; kk += 4) {
            float av[MI], bv[NT];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
              const int m = wave * MI + i;
              av[i] = Xs[(((m / TH + od) * PH + m % TH + oh) * PW + lc + ow) * kPS + kk + lk];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) bv[j] = Ws[(t * kCK + kk + lk) * WS + 16 * j + lc];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
              for (int j = 0; j < NT; ++j) part[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], part[i][j], 0, 0, 0);
          }
        }
      } else {
#pragma unroll
        for (int t = 0; t < kStepTaps; ++t) {
          const int kh = t / 3, kw = t % 3;
#pragma unroll
          for (int kk = 0; kk < kCK; kk += 4) {
            float av[MI], bv[NT];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
              const int m = wave * MI + i;
              const int col = MODE == kConvS2 ? (kw & 1) * kEven + lc + (kw >> 1) : lc + kw;
              av[i] = Xs[((((m / TH) * S + s) * PH + (m % TH) * S + kh) * PW + col) * kPS + kk + lk];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) bv[j] = Ws[(t * kCK + kk + lk) * WS + 16 * j + lc];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
              for (int j = 0; j < NT; ++j) part[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], part[i][j], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] += part[i][j];
  }
  // D layout: lane holds rows (voxels of the tile row) 4 (lane >> 4) .. + 3 of column (output channel) lane & 15
  const size_t out0 = (size_t)blockIdx.z * a.Do * a.Ho * a.Wo;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = wave * MI + i;
    int d = d0 + m / TH, h = h0 + m % TH;
    if (MODE == kDeconv) {
      if (d >= a.D || h >= a.H) continue;
      d = 2 * d + pd;
      h = 2 * h + ph;
    } else if (d >= a.Do || h >= a.Ho) {
      continue;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + 16 * j + lc;
      if (n >= a.Cout) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int w = w0 + 4 * lk + r;
        if (MODE == kDeconv) {
          if (w >= a.W) continue;
          w = 2 * w + pw;
        } else if (w >= a.Wo) {
          continue;
        }
        const size_t at = (out0 + ((size_t)d * a.Ho + h) * a.Wo + w) * a.Cout + n;
        float v = acc[i][j][r];
        if (a.relu) v = fmaxf(v, 0.0f);
        if (a.addend) v += a.addend[at];
        a.y[at] = v;
      }
    }
  }
}

template <int MODE, int NT> constexpr int patch_floats() { return Tile<MODE>::PD * Tile<MODE>::PH * Tile<MODE>::PW * kPS; }

template <int STRIDE, int NT>
__global__ __launch_bounds__(kThreads) void k_conv3d(Conv3dArgs a) {
  constexpr int MODE = STRIDE == 1 ? kConvS1 : kConvS2;
  __shared__ __attribute__((aligned(16))) float Xs[patch_floats<MODE, NT>()];
  __shared__ __attribute__((aligned(16))) float Ws[kStepTaps * kCK * weight_stride<NT>()];
  conv3d_body<MODE, NT>(a, Xs, Ws);
}

template <int NT>
__global__ __launch_bounds__(kThreads) void k_deconv3d_s2(Conv3dArgs a) {
  __shared__ __attribute__((aligned(16))) float Xs[patch_floats<kDeconv, NT>()];
  __shared__ __attribute__((aligned(16))) float Ws[8 * kCK * weight_stride<NT>()];
  conv3d_body<kDeconv, NT>(a, Xs, Ws);
}

// ---- the two thin layers of the net: conv0 (Cin 1) and prob (Cout 1), stride 1 ---------------------------------------------------------
// Both are bandwidth-bound, and the fp32 MFMA rate equals the vector rate, so the matrix unit buys nothing here while a 16 x 16 x 4 tile
// wastes 7/8 of its K on Cin 1 and 15/16 of its columns on Cout 1.  Plain fmaf chains in the SAME K order as k_conv3d (one chunk: taps
// (kd, kh, kw) ascending, then channel) and the same epilogue.  A workgroup is 64 voxels along W x 4 along H; a thread computes kThinD
// outputs along D from the kThinD + 2 input slabs, each read once, the weights of the pack (row k of tap t, column n) come from LDS.
// Index arithmetic is 32-bit: the launcher takes this route only for samples of fewer than 2^31 elements.  Measured against k_conv3d on
// the same layers in DESIGN.md 8n.
constexpr int kThinD = 4;

struct ThinAt {
  int w, h, n, d0;
  bool hok[3], wok[3];
};

__device__ __forceinline__ bool thin_at(const Conv3dArgs& a, int dblocks, ThinAt* t) {
  t->w = (int)blockIdx.x * 64 + (threadIdx.x & 63);
  t->h = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
  t->n = (int)blockIdx.z / dblocks;
  t->d0 = ((int)blockIdx.z % dblocks) * kThinD;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t->hok[k] = t->h + k - 1 >= 0 && t->h + k - 1 < a.H;
    t->wok[k] = t->w + k - 1 >= 0 && t->w + k - 1 < a.W;
  }
  return t->w < a.W && t->h < a.H;
}

template <int CO>       // Cin == 1, Cout <= CO <= 16
__global__ __launch_bounds__(kThreads) void k_conv3d_cin1(Conv3dArgs a, int dblocks, int vec) {
  __shared__ __attribute__((aligned(16))) float Wsh[27 * CO];
  for (int e = threadIdx.x; e < 27 * CO; e += kThreads) Wsh[e] = a.w[(size_t)(e / CO) * kCK * a.CoutPad + e % CO];
  __syncthreads();
  ThinAt t;
  if (!thin_at(a, dblocks, &t)) return;
  const float* x = a.x + (size_t)t.n * a.D * a.H * a.W;
  float acc[kThinD][CO], bias[CO];                                        // the chunk's chain starts at zero; the bias takes its sum, as in k_conv3d
#pragma unroll
  for (int n = 0; n < CO; ++n) {
    bias[n] = (a.bias && n < a.Cout) ? a.bias[n] : 0.0f;
#pragma unroll
    for (int od = 0; od < kThinD; ++od) acc[od][n] = 0.0f;
  }
#pragma unroll 1                                                          // a real loop: unrolled, every slab's loads and weights would be live at once
  for (int dz = 0; dz < kThinD + 2; ++dz) {                               // slab d0 + dz - 1 serves output od through kd = dz - od
    const int dd = t.d0 + dz - 1;
    const bool dok = dd >= 0 && dd < a.D;
    float v[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      v[j] = 0.0f;
      if (dok && t.hok[j / 3] && t.wok[j % 3]) v[j] = x[(dd * a.H + t.h + j / 3 - 1) * a.W + t.w + j % 3 - 1];
    }
#pragma unroll
    for (int od = 0; od < kThinD; ++od) {
      const int kd = dz - od;
      if (kd < 0 || kd > 2) continue;
#pragma unroll
      for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int n = 0; n < CO; ++n) acc[od][n] = fmaf(v[j], Wsh[(kd * 9 + j) * CO + n], acc[od][n]);
    }
  }
#pragma unroll
  for (int od = 0; od < kThinD; ++od) {
    const int d = t.d0 + od;
    if (d >= a.D) continue;
    const size_t at = ((((size_t)t.n * a.D + d) * a.H + t.h) * a.W + t.w) * a.Cout;
    if (vec) {                                                            // Cout == CO, y and the addend 16-byte aligned
#pragma unroll
      for (int n = 0; n < CO; n += 4) {
        v4f r = (v4f){bias[n] + acc[od][n], bias[n + 1] + acc[od][n + 1], bias[n + 2] + acc[od][n + 2], bias[n + 3] + acc[od][n + 3]};
        if (a.relu) r = (v4f){fmaxf(r[0], 0.0f), fmaxf(r[1], 0.0f), fmaxf(r[2], 0.0f), fmaxf(r[3], 0.0f)};
        if (a.addend) r += *reinterpret_cast<const v4f*>(a.addend + at + n);
        *reinterpret_cast<v4f*>(a.y + at + n) = r;
      }
    } else {
#pragma unroll
      for (int n = 0; n < CO; ++n) {
        if (n >= a.Cout) continue;
        float r = bias[n] + acc[od][n];
        if (a.relu) r = fmaxf(r, 0.0f);
        if (a.addend) r += a.addend[at + n];
        a.y[at + n] = r;
      }
    }
  }
}

template <int CI>       // Cin == CI (4 or 8: one chunk), Cout == 1, x 16-byte aligned
__global__ __launch_bounds__(kThreads) void k_conv3d_cout1(Conv3dArgs a, int dblocks) {
  __shared__ __attribute__((aligned(16))) float Wsh[27 * CI];
  for (int e = threadIdx.x; e < 27 * CI; e += kThreads) Wsh[e] = a.w[((size_t)(e / CI) * kCK + e % CI) * a.CoutPad];
  __syncthreads();
  ThinAt t;
  if (!thin_at(a, dblocks, &t)) return;
  const float* x = a.x + (size_t)t.n * a.D * a.H * a.W * CI;
  const float b = a.bias ? a.bias[0] : 0.0f;
  float acc[kThinD];
#pragma unroll
  for (int od = 0; od < kThinD; ++od) acc[od] = 0.0f;                   // the chain starts at zero; the bias takes its sum, as in k_conv3d
#pragma unroll 1                                                          // a real loop: see k_conv3d_cin1
  for (int dz = 0; dz < kThinD + 2; ++dz) {                               // slab d0 + dz - 1 serves output od through kd = dz - od
    const int dd = t.d0 + dz - 1;
    const bool dok = dd >= 0 && dd < a.D;
    v4f v[9][CI / 4];
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int q = 0; q < CI / 4; ++q) {
        v[j][q] = (v4f){0.f, 0.f, 0.f, 0.f};
        if (dok && t.hok[j / 3] && t.wok[j % 3])
          v[j][q] = *reinterpret_cast<const v4f*>(x + (size_t)((dd * a.H + t.h + j / 3 - 1) * a.W + t.w + j % 3 - 1) * CI + 4 * q);
      }
#pragma unroll
    for (int od = 0; od < kThinD; ++od) {
      const int kd = dz - od;
      if (kd < 0 || kd > 2) continue;
#pragma unroll
      for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int k = 0; k < CI; ++k) acc[od] = fmaf(v[j][k / 4][k % 4], Wsh[(kd * 9 + j) * CI + k], acc[od]);
    }
  }
#pragma unroll
  for (int od = 0; od < kThinD; ++od) {
    const int d = t.d0 + od;
    if (d >= a.D) continue;
    const size_t at = (((size_t)t.n * a.D + d) * a.H + t.h) * a.W + t.w;
    float r = b + acc[od];
    if (a.relu) r = fmaxf(r, 0.0f);
    if (a.addend) r += a.addend[at];
    a.y[at] = r;
  }
}

int cout_pad(int Cout) { return Cout <= 16 ? 16 : Cout <= 32 ? 32 : (Cout + 63) / 64 * 64; }

int check_volume(const char* who, int N, int D, int H, int W, int C) {
  DINER_CHECK_ARG(N >= 1 && D >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: N, D, H, W, C = %d, %d, %d, %d, %d (each must be >= 1)", who, N, D, H, W, C);
  // factor by factor: the product of five ints near 2^31 does not fit in 64 bits
  long long room = 1LL << 40;
  const int sizes[5] = {N, D, H, W, C};
  for (int k = 0; k < 5; ++k) room /= sizes[k];
  DINER_CHECK_ARG(room >= 1, "%s: %d x %d x %d x %d x %d elements are more than 2^40", who, N, D, H, W, C);
  return 0;
}

template <int MODE>
int launch(const char* who, const float* x, const float* wpack, const float* bias, const float* addend, float* y, int N, int D, int H, int W,
           int Cin, int Cout, int relu, void* stream) {
  using T = Tile<MODE>;
  int rc = check_volume(who, N, D, H, W, Cin);
  if (rc) return rc;
  DINER_CHECK_ARG(Cout >= 1, "%s: Cout = %d (must be >= 1)", who, Cout);
  DINER_CHECK_ARG(D <= (1 << 29) && H <= (1 << 29) && W <= (1 << 29), "%s: D, H, W = %d, %d, %d (each at most 2^29)", who, D, H, W);
  Conv3dArgs a;
  a.x = x; a.w = wpack; a.bias = bias; a.addend = addend; a.y = y;
  a.D = D; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.CoutPad = cout_pad(Cout);
  if (MODE == kDeconv) {
    a.Do = 2 * D; a.Ho = 2 * H; a.Wo = 2 * W;
  } else {
    a.Do = (D - 1) / T::S + 1; a.Ho = (H - 1) / T::S + 1; a.Wo = (W - 1) / T::S + 1;
  }
  rc = check_volume(who, N, a.Do, a.Ho, a.Wo, Cout);
  if (rc) return rc;
  DINER_CHECK_ARG(N <= 65535, "%s: N = %d samples (at most 65535 a call)", who, N);
  DINER_CHECK_ARG(x && wpack && y, "%s: null pointer argument", who);
  DINER_CHECK_ARG((reinterpret_cast<uintptr_t>(wpack) & 15) == 0, "%s: the packed weights are not 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  a.relu = relu != 0;
  const bool thin_shape = (Cin == 1 && Cout <= 16) || (Cout == 1 && (Cin == 4 || Cin == 8) && (reinterpret_cast<uintptr_t>(x) & 15) == 0);
  // 32-bit index arithmetic inside a sample and N x ceil(D / kThinD) as one grid dimension bound the thin route; beyond, the MFMA kernels
  const bool thin_size = (long long)D * H * W * Cin < (1LL << 31) && (long long)N * ((D + kThinD - 1) / kThinD) <= 65535 && H <= 4 * 65535;
  if (MODE == kConvS1 && thin_shape && thin_size) {
    // the thin layers: 64 x 4 x kThinD output voxels a workgroup
    const int dblocks = (D + kThinD - 1) / kThinD;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)(N * dblocks)), block(kThreads);
    if (Cin == 1) {
      const int co = Cout <= 4 ? 4 : Cout <= 8 ? 8 : 16;
      const int vec = Cout == co && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(addend)) & 15) == 0;
      if (co == 4) hipLaunchKernelGGL(k_conv3d_cin1<4>, grid, block, 0, st, a, dblocks, vec);
      else if (co == 8) hipLaunchKernelGGL(k_conv3d_cin1<8>, grid, block, 0, st, a, dblocks, vec);
      else hipLaunchKernelGGL(k_conv3d_cin1<16>, grid, block, 0, st, a, dblocks, vec);
    } else if (Cin == 4) {
      hipLaunchKernelGGL(k_conv3d_cout1<4>, grid, block, 0, st, a, dblocks);
    } else {
      hipLaunchKernelGGL(k_conv3d_cout1<8>, grid, block, 0, st, a, dblocks);
    }
    DINER_LAUNCH_OK();
    return 0;
  }
  // tiles: of the output for a convolution; of the input grid, times the eight parity classes, for the transposed layer
  const int td = MODE == kDeconv ? D : a.Do, th = MODE == kDeconv ? H : a.Ho, tw = MODE == kDeconv ? W : a.Wo;
  a.tiles_w = (tw + kTW - 1) / kTW;
  a.tiles_h = (th + T::TH - 1) / T::TH;
  const long long tiles = (long long)a.tiles_w * a.tiles_h * ((td + T::TD - 1) / T::TD) * (MODE == kDeconv ? 8 : 1);
  int nt = a.CoutPad == 16 ? 1 : a.CoutPad == 32 ? 2 : 4;
  // a small volume has few tiles: narrower workgroups, more of them, then fill more of the chip (an output's chain does not depend on NT)
  while (nt > 1 && tiles * (a.CoutPad / (16 * nt)) < kFillWorkgroups) nt >>= 1;
  const int groups = a.CoutPad / (16 * nt);
  DINER_CHECK_ARG(tiles < (1LL << 31) && groups <= 65535, "%s: %d x %d x %d voxels x %d channels are too many tiles", who, D, H, W, Cout);
  const dim3 grid((unsigned)tiles, (unsigned)groups, (unsigned)N), block(kThreads);
  if (MODE == kDeconv) {
    if (nt == 1) hipLaunchKernelGGL(k_deconv3d_s2<1>, grid, block, 0, st, a);
    else if (nt == 2) hipLaunchKernelGGL(k_deconv3d_s2<2>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_deconv3d_s2<4>, grid, block, 0, st, a);
  } else {
    constexpr int S = T::S;
    if (nt == 1) hipLaunchKernelGGL((k_conv3d<S, 1>), grid, block, 0, st, a);
    else if (nt == 2) hipLaunchKernelGGL((k_conv3d<S, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_conv3d<S, 4>), grid, block, 0, st, a);
  }
  DINER_LAUNCH_OK();
  return 0;
}

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" size_t diner_conv3d_pack_floats(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  return (size_t)((Cin + kCK - 1) / kCK) * 27 * kCK * (size_t)cout_pad(Cout);
}

extern "C" int diner_conv3d_f32(const float* x, const float* wpack, const float* bias, const float* addend, float* y, int N, int D, int H, int W,
                                int Cin, int Cout, int stride, int relu, void* stream) {
  DINER_CHECK_ARG(stride == 1 || stride == 2, "conv3d: stride = %d (must be 1 or 2)", stride);
  if (stride == 1) return launch<kConvS1>("conv3d", x, wpack, bias, addend, y, N, D, H, W, Cin, Cout, relu, stream);
  return launch<kConvS2>("conv3d", x, wpack, bias, addend, y, N, D, H, W, Cin, Cout, relu, stream);
}

extern "C" int diner_deconv3d_s2_f32(const float* x, const float* wpack, const float* bias, const float* addend, float* y, int N, int D, int H,
                                     int W, int Cin, int Cout, int relu, void* stream) {
  return launch<kDeconv>("deconv3d_s2", x, wpack, bias, addend, y, N, D, H, W, Cin, Cout, relu, stream);
}
