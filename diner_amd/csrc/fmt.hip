// The depth estimator's feature transformer on the device (diner_amd/mvs.py, DeviceFMT / DeviceFMTWithPathway): TransMVSNet's FMT
// (models/FMT.py), eight linear-attention encoder layers of d_model 32, 8 heads of 4, d_ff 64 on the quarter-resolution features, and the
// FPN pathway that carries the result into stages 2 and 3.  Everything fp32; activations are channels-last tokens (N, L = H W, 32).
//   * k_fmt_tokenise: (N,32,H,W) NCHW + the top-left H x W crop of the sine positional encoding -> tokens, through an LDS transpose.
//   * k_fmt_kv: the attention state of a layer's source tokens.  K = elu(src Wk^T + bk) + 1, V = src Wv^T + bv, per head
//     KV[m][d] = sum_s K[s,d] V[s,m] and Ksum[d] = sum_s K[s,d]: 8 x (16 + 4) = 160 numbers an image.  K and V never reach memory.  A
//     workgroup sums a fixed run of DINER_FMT_KV_TOKENS tokens (products and sums in double: the lanes' xor tree, then the waves in
//     order) and writes 160 doubles; k_fmt_kv_finalise adds the partials in block order and rounds once.  No atomics: the order is fixed
//     by the shape alone.
//   * k_fmt_layer: one encoder layer, strictly per token, one thread a token: Q = elu(x Wq^T + bq) + 1; per head Z = 1 / (Q . Ksum + 1e-6),
//     A[m] = Z sum_d Q[d] KV[m][d]; x1 = LN1(x + A Wo^T + bo); y = relu(x1 W1^T + b1) W2^T + b2; out = LN2(x1 + y).  LayerNorm as in
//     torch: biased variance, eps 1e-5, affine.  The four GEMMs (K = 32, 32, 32, 64) are plain fmaf chains: every output is the bias plus
//     ONE chain over k ascending.  The fp32 MFMA has the vector rate, and a thread a token needs no cross-lane step for the attention or
//     the LayerNorms; the weights (24 KB, transposed in the pack) sit in LDS and are read as broadcasts, the token's activations go
//     through an LDS column of its own so that the k loop stays a loop (no dynamic register index, no scratch).
//   * k_fpn_reduce / k_fpn_merge: y = bilinear2x(conv1x1(top)) + lateral, the 1 x 1 at the coarse size in its own launch.
// A workgroup never crosses images (blockIdx.y is the image), so an image's bits do not depend on its place in the batch or on how many
// images share the launch.
#include <cstdint>
#include "common.hpp"

namespace diner {
namespace {

constexpr int kD = DINER_FMT_D_MODEL;              // 32
constexpr int kFF = DINER_FMT_D_FF;                // 64
constexpr int kHeads = DINER_FMT_NHEAD;            // 8
constexpr int kHd = kD / kHeads;                   // 4
constexpr int kState = DINER_FMT_STATE_FLOATS;     // 160
constexpr int kKvTokens = DINER_FMT_KV_TOKENS;     // 512
constexpr int kKvThreads = 256;
constexpr int kKvPerThread = kKvTokens / kKvThreads;
constexpr int kLayerTokens = 128;                  // tokens (= threads) of one k_fmt_layer workgroup
constexpr int kTokTile = 64;                       // tokens of one k_fmt_tokenise workgroup

// the layer pack (ops.pack_fmt_layer): the matrices TRANSPOSED, [k][out], then the vectors
constexpr int oWq = 0, oWk = 1024, oWv = 2048, oWo = 3072, oW1 = 4096, oW2 = 6144, oVec = 8192;
constexpr int vBq = 0, vBk = 32, vBv = 64, vBo = 96, vG1 = 128, vBe1 = 160, vB1 = 192, vB2 = 256, vG2 = 288, vBe2 = 320, kVec = 352;
static_assert(oVec + kVec == DINER_FMT_PACK_FLOATS, "pack layout");
static_assert(kHd == 4 && kD == 32 && kFF == 64 && kState == kHeads * (kHd * kHd + kHd), "the kernels are written for d_model 32, 8 heads, d_ff 64");

__device__ __forceinline__ float elu1(float v) { return (v > 0.0f ? v : expm1f(v)) + 1.0f; }

__global__ __launch_bounds__(256) void k_fmt_tokenise(const float* __restrict__ x, const float* __restrict__ pe, float* __restrict__ tok, int H,
                                                       int W, int pe_h, int pe_w) {
  __shared__ float Ts[kTokTile * (kD + 1)];
  const int tid = threadIdx.x, L = H * W, l0 = (int)blockIdx.x * kTokTile;
  const size_t n = blockIdx.y;
  {
    const int li = tid & 63, l = l0 + li;
    if (l < L) {
      const int py = l / W, px = l % W;
#pragma unroll
      for (int i = 0; i < kD / 4; ++i) {
        const int c = (tid >> 6) + 4 * i;
        Ts[li * (kD + 1) + c] = x[(n * kD + c) * L + l] + pe[((size_t)c * pe_h + py) * pe_w + px];       // one fp32 add, as torch's
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kTokTile * kD / 256; ++i) {
    const int e = tid + 256 * i, li = e >> 5, c = e & 31;
    if (l0 + li < L) tok[(n * L + l0 + li) * kD + c] = Ts[li * (kD + 1) + c];
  }
}

__global__ __launch_bounds__(kKvThreads) void k_fmt_kv(const float* __restrict__ src, const float* __restrict__ pack,
                                                        double* __restrict__ partials, int L, int nblk) {
  __shared__ __attribute__((aligned(16))) float Wk[kD * kD];
  __shared__ __attribute__((aligned(16))) float Wv[kD * kD];
  __shared__ float Bk[kD], Bv[kD];
  __shared__ double red[kKvThreads / 64][kState];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = blockIdx.y;
  const int blk = blockIdx.x;
  reinterpret_cast<v4f*>(Wk)[tid] = reinterpret_cast<const v4f*>(pack + oWk)[tid];
  reinterpret_cast<v4f*>(Wv)[tid] = reinterpret_cast<const v4f*>(pack + oWv)[tid];
  if (tid < kD) {
    Bk[tid] = pack[oVec + vBk + tid];
    Bv[tid] = pack[oVec + vBv + tid];
  }
  float x[kKvPerThread][kD];
  bool ok[kKvPerThread];
#pragma unroll
  for (int t = 0; t < kKvPerThread; ++t) {
    const int l = blk * kKvTokens + t * kKvThreads + tid;
    ok[t] = l < L;
#pragma unroll
    for (int q = 0; q < kD / 4; ++q) {
      v4f v = (v4f){0.f, 0.f, 0.f, 0.f};
      if (ok[t]) v = *reinterpret_cast<const v4f*>(src + (n * L + l) * kD + 4 * q);
      x[t][4 * q] = v[0]; x[t][4 * q + 1] = v[1]; x[t][4 * q + 2] = v[2]; x[t][4 * q + 3] = v[3];
    }
  }
  __syncthreads();
#pragma unroll 1                                                         // a real loop: one head's twenty sums are live at a time
  for (int h = 0; h < kHeads; ++h) {
    double acc[kHd * kHd + kHd];
#pragma unroll
    for (int i = 0; i < kHd * kHd + kHd; ++i) acc[i] = 0.0;
#pragma unroll
    for (int t = 0; t < kKvPerThread; ++t) {
      float kq[kHd], vq[kHd];
#pragma unroll
      for (int i = 0; i < kHd; ++i) {
        kq[i] = Bk[h * kHd + i];
        vq[i] = Bv[h * kHd + i];
      }
#pragma unroll
      for (int k = 0; k < kD; ++k) {
        const v4f wk = *reinterpret_cast<const v4f*>(&Wk[k * kD + h * kHd]);
        const v4f wv = *reinterpret_cast<const v4f*>(&Wv[k * kD + h * kHd]);
#pragma unroll
        for (int i = 0; i < kHd; ++i) {
          kq[i] = fmaf(x[t][k], wk[i], kq[i]);
          vq[i] = fmaf(x[t][k], wv[i], vq[i]);
        }
      }
#pragma unroll
      for (int d = 0; d < kHd; ++d) {
        const double kd = ok[t] ? (double)elu1(kq[d]) : 0.0;            // a token beyond L adds +0
#pragma unroll
        for (int m = 0; m < kHd; ++m) acc[m * kHd + d] = fma(kd, (double)vq[m], acc[m * kHd + d]);
        acc[kHd * kHd + d] += kd;
      }
    }
#pragma unroll
    for (int i = 0; i < kHd * kHd + kHd; ++i) {
      const double s = wave_sum_d(acc[i]);
      const int at = i < kHd * kHd ? h * kHd * kHd + i : kHeads * kHd * kHd + h * kHd + (i - kHd * kHd);
      if (lane == 0) red[wave][at] = s;
    }
  }
  __syncthreads();
  if (tid < kState) {
    double s = red[0][tid];
#pragma unroll
    for (int w = 1; w < kKvThreads / 64; ++w) s += red[w][tid];
    partials[(n * nblk + blk) * kState + tid] = s;
  }
}

__global__ __launch_bounds__(192) void k_fmt_kv_finalise(const double* __restrict__ partials, float* __restrict__ state, int nblk) {
  const int v = threadIdx.x;
  const size_t n = blockIdx.x;
  if (v >= kState) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partials[(n * nblk + b) * kState + v];      // block order
  state[n * kState + v] = (float)s;
}

// acc[j] = bias[j] + sum_k Xs[k][token] Wt[k][j], one fmaf chain an output, k ascending
template <int NOUT, int NIN>
__device__ __forceinline__ void token_gemm(const float* Xs, const float* Wt, const float* bias, float* acc) {
#pragma unroll
  for (int j = 0; j < NOUT; ++j) acc[j] = bias[j];
#pragma unroll 2
  for (int k = 0; k < NIN; ++k) {
    const float xv = Xs[k * kLayerTokens];
#pragma unroll
    for (int j = 0; j < NOUT; j += 4) {
      const v4f w = *reinterpret_cast<const v4f*>(&Wt[k * NOUT + j]);
      acc[j] = fmaf(xv, w[0], acc[j]);
      acc[j + 1] = fmaf(xv, w[1], acc[j + 1]);
      acc[j + 2] = fmaf(xv, w[2], acc[j + 2]);
      acc[j + 3] = fmaf(xv, w[3], acc[j + 3]);
    }
  }
}

// torch's LayerNorm over the 32 channels: biased variance, eps 1e-5, affine
__device__ __forceinline__ void layer_norm(float* v, const float* gamma, const float* beta) {
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < kD; ++j) s += v[j];
  const float mean = s * (1.0f / kD);
  float q = 0.0f;
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    const float d = v[j] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(q * (1.0f / kD) + 1e-5f);
#pragma unroll
  for (int j = 0; j < kD; ++j) v[j] = fmaf((v[j] - mean) * rstd, gamma[j], beta[j]);
}

__global__ __launch_bounds__(kLayerTokens) void k_fmt_layer(const float* __restrict__ x, const float* __restrict__ pack,
                                                             const float* __restrict__ state, float* __restrict__ out, int L, int state_mod) {
  __shared__ __attribute__((aligned(16))) float Wq[kD * kD];
  __shared__ __attribute__((aligned(16))) float Wo[kD * kD];
  __shared__ __attribute__((aligned(16))) float W1[kD * kFF];
  __shared__ __attribute__((aligned(16))) float W2[kFF * kD];
  __shared__ __attribute__((aligned(16))) float Vs[kVec];
  __shared__ float St[kState];
  __shared__ float Xs[kFF * kLayerTokens];                               // the token's activations: column tid, row k
  const int tid = threadIdx.x;
  const size_t n = blockIdx.y;
  const int l = (int)blockIdx.x * kLayerTokens + tid;
  const bool live = l < L;
  for (int e = tid; e < kD * kD / 4; e += kLayerTokens) {
    reinterpret_cast<v4f*>(Wq)[e] = reinterpret_cast<const v4f*>(pack + oWq)[e];
    reinterpret_cast<v4f*>(Wo)[e] = reinterpret_cast<const v4f*>(pack + oWo)[e];
  }
  for (int e = tid; e < kD * kFF / 4; e += kLayerTokens) {
    reinterpret_cast<v4f*>(W1)[e] = reinterpret_cast<const v4f*>(pack + oW1)[e];
    reinterpret_cast<v4f*>(W2)[e] = reinterpret_cast<const v4f*>(pack + oW2)[e];
  }
  for (int e = tid; e < kVec; e += kLayerTokens) Vs[e] = pack[oVec + e];
  for (int e = tid; e < kState; e += kLayerTokens) St[e] = state[(n % (size_t)state_mod) * kState + e];
  float* col = Xs + tid;
  float xin[kD];
#pragma unroll
  for (int q = 0; q < kD / 4; ++q) {
    v4f v = (v4f){0.f, 0.f, 0.f, 0.f};
    if (live) v = *reinterpret_cast<const v4f*>(x + (n * L + l) * kD + 4 * q);
    xin[4 * q] = v[0]; xin[4 * q + 1] = v[1]; xin[4 * q + 2] = v[2]; xin[4 * q + 3] = v[3];
  }
#pragma unroll
  for (int k = 0; k < kD; ++k) col[k * kLayerTokens] = xin[k];
  __syncthreads();                                                       // the only barrier: from here on a thread reads its own column

  float a[kD];
  token_gemm<kD, kD>(col, Wq, Vs + vBq, a);
#pragma unroll
  for (int j = 0; j < kD; ++j) a[j] = elu1(a[j]);
#pragma unroll
  for (int h = 0; h < kHeads; ++h) {
    float den = 0.0f;
#pragma unroll
    for (int d = 0; d < kHd; ++d) den = fmaf(a[h * kHd + d], St[kHeads * kHd * kHd + h * kHd + d], den);
    const float z = 1.0f / (den + 1e-6f);
#pragma unroll
    for (int m = 0; m < kHd; ++m) {
      float s = 0.0f;
#pragma unroll
      for (int d = 0; d < kHd; ++d) s = fmaf(a[h * kHd + d], St[(h * kHd + m) * kHd + d], s);
      col[(h * kHd + m) * kLayerTokens] = s * z;                         // Q is read in full before row h kHd + m is overwritten: a[] holds it
    }
  }
  token_gemm<kD, kD>(col, Wo, Vs + vBo, a);
#pragma unroll
  for (int j = 0; j < kD; ++j) xin[j] += a[j];
  layer_norm(xin, Vs + vG1, Vs + vBe1);                                  // xin: x1 from here on
#pragma unroll
  for (int k = 0; k < kD; ++k) col[k * kLayerTokens] = xin[k];
  float hdn[kFF];
  token_gemm<kFF, kD>(col, W1, Vs + vB1, hdn);
#pragma unroll
  for (int k = 0; k < kFF; ++k) col[k * kLayerTokens] = fmaxf(hdn[k], 0.0f);
  token_gemm<kD, kFF>(col, W2, Vs + vB2, a);
#pragma unroll
  for (int j = 0; j < kD; ++j) xin[j] += a[j];
  layer_norm(xin, Vs + vG2, Vs + vBe2);
  if (live) {
#pragma unroll
    for (int q = 0; q < kD / 4; ++q)
      *reinterpret_cast<v4f*>(out + (n * L + l) * kD + 4 * q) = (v4f){xin[4 * q], xin[4 * q + 1], xin[4 * q + 2], xin[4 * q + 3]};
  }
}

// ---- the pathway ------------------------------------------------------------------------------------------------------------------------
constexpr int kFpnMaxC = DINER_FPN_MAX_CHANNELS;   // 64

// the 1 x 1 convolution at the coarse size: red[p][co] = sum_k top[p][k] w[co][k], one chain, k ascending
__global__ __launch_bounds__(256) void k_fpn_reduce(const float* __restrict__ top, const float* __restrict__ w, float* __restrict__ red,
                                                     long long total, int Ctop, int Clat) {
  __shared__ float Ws[kFpnMaxC * (kFpnMaxC + 1)];
  for (int e = threadIdx.x; e < Clat * Ctop; e += 256) Ws[(e / Ctop) * (Ctop + 1) + e % Ctop] = w[e];
  __syncthreads();
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int co = (int)(e % Clat);
  const float* t = top + (e / Clat) * Ctop;
  float acc = 0.0f;
  for (int k = 0; k < Ctop; ++k) acc = fmaf(t[k], Ws[co * (Ctop + 1) + k], acc);
  red[e] = acc;
}

// F.interpolate(mode="bilinear", align_corners=False) to exactly twice the size: source coordinate max(0.5 (o + 0.5) - 0.5, 0), so the
// phases are 0.25 / 0.75 and the first and last output copy the edge
__device__ __forceinline__ void up2_taps(int o, int n_in, int* i0, int* i1, float* l0, float* l1) {
  const float s = fmaxf(0.5f * ((float)o + 0.5f) - 0.5f, 0.0f);
  *i0 = (int)s;
  *i1 = *i0 + (*i0 < n_in - 1 ? 1 : 0);
  *l1 = s - (float)*i0;
  *l0 = 1.0f - *l1;
}

__global__ __launch_bounds__(256) void k_fpn_merge(const float* __restrict__ red, const float* __restrict__ lat, float* __restrict__ y,
                                                    long long total, int H, int W, int Clat) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;       // one thread: four channels of one output pixel
  if (e >= total) return;
  const int quads = Clat / 4, q = (int)(e % quads);
  long long pix = e / quads;
  const int ox = (int)(pix % (2 * W));
  pix /= 2 * W;
  const int oy = (int)(pix % (2 * H));
  const long long n = pix / (2 * H);
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  up2_taps(oy, H, &y0, &y1, &ly0, &ly1);
  up2_taps(ox, W, &x0, &x1, &lx0, &lx1);
  const float* r = red + n * H * W * Clat + 4 * q;
  const v4f p00 = *reinterpret_cast<const v4f*>(r + ((long long)y0 * W + x0) * Clat), p01 = *reinterpret_cast<const v4f*>(r + ((long long)y0 * W + x1) * Clat);
  const v4f p10 = *reinterpret_cast<const v4f*>(r + ((long long)y1 * W + x0) * Clat), p11 = *reinterpret_cast<const v4f*>(r + ((long long)y1 * W + x1) * Clat);
  const v4f up = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
  *reinterpret_cast<v4f*>(y + 4 * e) = up + *reinterpret_cast<const v4f*>(lat + 4 * e);
}

int check_tokens(const char* who, int N, int L) {
  DINER_CHECK_ARG(N >= 1 && N <= 65535, "%s: N = %d images (must be in [1, 65535])", who, N);
  DINER_CHECK_ARG(L >= 1 && L <= DINER_FMT_MAX_HW * DINER_FMT_MAX_HW, "%s: L = %d tokens (must be in [1, %d])", who, L,
                  DINER_FMT_MAX_HW * DINER_FMT_MAX_HW);
  return 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" size_t diner_fmt_pack_floats(void) { return DINER_FMT_PACK_FLOATS; }

extern "C" size_t diner_fmt_kv_blocks(int L) { return L < 1 ? 0 : (size_t)((L + kKvTokens - 1) / kKvTokens); }

extern "C" int diner_fmt_tokenise_f32(const float* x, const float* pe, float* tokens, int N, int C, int H, int W, int pe_h, int pe_w, void* stream) {
  DINER_CHECK_ARG(C == kD, "fmt_tokenise: C = %d channels (the kernels are built for d_model %d)", C, kD);
  DINER_CHECK_ARG(H >= 1 && W >= 1 && H <= DINER_FMT_MAX_HW && W <= DINER_FMT_MAX_HW, "fmt_tokenise: H, W = %d, %d (each must be in [1, %d])", H,
                  W, DINER_FMT_MAX_HW);
  DINER_CHECK_ARG(pe_h >= H && pe_w >= W && pe_h <= DINER_FMT_MAX_HW && pe_w <= DINER_FMT_MAX_HW,
                  "fmt_tokenise: the positional encoding is %d x %d, the map %d x %d (it must cover the map, at most %d a side)", pe_h, pe_w, H, W,
                  DINER_FMT_MAX_HW);
  int rc = check_tokens("fmt_tokenise", N, H * W);
  if (rc) return rc;
  DINER_CHECK_ARG(x && pe && tokens, "fmt_tokenise: null pointer argument");
  const dim3 grid((unsigned)((H * W + kTokTile - 1) / kTokTile), (unsigned)N), block(256);
  hipLaunchKernelGGL(k_fmt_tokenise, grid, block, 0, (hipStream_t)stream, x, pe, tokens, H, W, pe_h, pe_w);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_fmt_kv_f32(const float* src, const float* pack, double* partials, float* state, int N, int L, void* stream) {
  int rc = check_tokens("fmt_kv", N, L);
  if (rc) return rc;
  DINER_CHECK_ARG(src && pack && partials && state, "fmt_kv: null pointer argument");
  DINER_CHECK_ARG(aligned16(src) && aligned16(pack), "fmt_kv: the tokens and the pack must be 16-byte aligned");
  DINER_CHECK_ARG((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "fmt_kv: the partial sums must be 8-byte aligned");
  const int nblk = (L + kKvTokens - 1) / kKvTokens;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_fmt_kv, dim3((unsigned)nblk, (unsigned)N), dim3(kKvThreads), 0, st, src, pack, partials, L, nblk);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_fmt_kv_finalise, dim3((unsigned)N), dim3(192), 0, st, (const double*)partials, state, nblk);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_fmt_layer_f32(const float* x, const float* pack, const float* state, float* out, int N, int L, int state_rows, void* stream) {
  int rc = check_tokens("fmt_layer", N, L);
  if (rc) return rc;
  DINER_CHECK_ARG(state_rows >= 1 && state_rows <= N && N % state_rows == 0,
                  "fmt_layer: state_rows = %d (must divide N = %d: image n reads row n mod state_rows)", state_rows, N);
  DINER_CHECK_ARG(x && pack && state && out, "fmt_layer: null pointer argument");
  DINER_CHECK_ARG(aligned16(x) && aligned16(pack) && aligned16(out), "fmt_layer: the tokens and the pack must be 16-byte aligned");
  const dim3 grid((unsigned)((L + kLayerTokens - 1) / kLayerTokens), (unsigned)N), block(kLayerTokens);
  hipLaunchKernelGGL(k_fmt_layer, grid, block, 0, (hipStream_t)stream, x, pack, state, out, L, state_rows);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_fpn_merge_f32(const float* top, const float* w, const float* lateral, float* reduced, float* y, int N, int H, int W, int Ctop,
                                   int Clat, void* stream) {
  int rc = check_nhwc("fpn_merge", N, H, W, Ctop);
  if (rc) return rc;
  DINER_CHECK_ARG(Ctop <= kFpnMaxC && Clat >= 4 && Clat <= kFpnMaxC && Clat % 4 == 0,
                  "fpn_merge: Ctop = %d, Clat = %d (Ctop at most %d, Clat a multiple of 4 in [4, %d])", Ctop, Clat, kFpnMaxC, kFpnMaxC);
  DINER_CHECK_ARG(H <= (1 << 14) && W <= (1 << 14), "fpn_merge: H, W = %d, %d (each at most 2^14)", H, W);
  const long long fine = (long long)N * (2 * H) * (2 * W) * (Clat / 4), coarse = (long long)N * H * W * Clat;
  DINER_CHECK_ARG((fine + 255) / 256 < (1LL << 31), "fpn_merge: %d x %d x %d x %d outputs are too many for one launch", N, 2 * H, 2 * W, Clat);
  DINER_CHECK_ARG(top && w && lateral && reduced && y, "fpn_merge: null pointer argument");
  DINER_CHECK_ARG(aligned16(lateral) && aligned16(reduced) && aligned16(y), "fpn_merge: lateral, reduced and y must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_fpn_reduce, dim3((unsigned)((coarse + 255) / 256)), dim3(256), 0, st, top, w, reduced, coarse, Ctop, Clat);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_fpn_merge, dim3((unsigned)((fine + 255) / 256)), dim3(256), 0, st, (const float*)reduced, lateral, y, fine, H, W, Clat);
  DINER_LAUNCH_OK();
  return 0;
}
