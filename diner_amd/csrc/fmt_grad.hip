// The backward pass of one FMT encoder layer (fmt.hip's k_fmt_kv + k_fmt_layer; diner_amd/mvs.py, fmt_layer).  Everything fp32, sums that
// cross tokens in a fixed order, no atomics anywhere: every output has the same bits on every run, and a tile never crosses images.
//   * k_fmt_grad_query: one thread a token, 128 tokens a tile.  It recomputes the forward from x and the 160-float state with fmt.hip's own
//     fmaf chains (nothing else is saved), then walks back: LN2, the feed-forward, LN1, the out projection, the attention's query side.
//     The weights sit in LDS in the pack's [k][out] layout, which serves Y = X W^T (a chain over k, the token's activations read from its
//     LDS column) and dX = dY W (dY in registers, a loop over k that writes row k of the column): no second copy, no dynamic register
//     index.  The token's activations go through column `As`, its gradients through column `Gs`; a parameter gradient is the sum over
//     the tile's tokens of an outer product of the two columns, formed by all 128 threads as fmaf chains in token order (each thread a
//     4 x 2 or 4 x 4 patch of the matrix) and added to the workgroup's slab.  d_x is written once per element.  The tile's share of d_state
//     is 160 doubles (products in double, the lanes' xor tree, then the two waves in order).
//   * k_fmt_grad_state: d_state (R,160) = the tiles' shares in (image, tile) order over the images that read the row, in double, rounded once.
//   * k_fmt_grad_source: one thread a source token: recomputes kp, K, V, forms dK, dV from d_state, d_src = dkp Wk + dV Wv, written once
//     (or, for a self layer, added to the d_x the query kernel wrote: the launches are ordered and one thread owns the element), and
//     the slabs of Wk bk Wv bv.
//   * k_fmt_grad_finish: the slabs of each parameter element in slab order in double, rounded once, in torch's (out, in) layout.
// A workgroup walks a fixed run of consecutive tiles (tiles / slabs, rounded up).  A tile's sums are chains from 0 over its 128 tokens; the
// slab adds them tile by tile as a (sum, carry) pair of floats (two-sum), so a slab of many tiles is as exact as many slabs of one: a
// plain float chain over 2080 tokens was measured at 2.5 to 5.3 times the bar on the bias sums.
#include <cstdint>
#include <mutex>
#include "common.hpp"

namespace diner {
namespace {

constexpr int kD = DINER_FMT_D_MODEL;              // 32
constexpr int kFF = DINER_FMT_D_FF;                // 64
constexpr int kHeads = DINER_FMT_NHEAD;            // 8
constexpr int kHd = kD / kHeads;                   // 4
constexpr int kState = DINER_FMT_STATE_FLOATS;     // 160
constexpr int kTok = DINER_FMT_GRAD_TOKENS;        // 128 tokens (= threads) of a tile
constexpr int kLd = kTok + 4;                      // row stride of a column block: rows stay 16-byte aligned and start 4 banks apart
constexpr int kQSlab = DINER_FMT_GRAD_QUERY_SLAB_FLOATS;    // 6432
constexpr int kSSlab = DINER_FMT_GRAD_SOURCE_SLAB_FLOATS;   // 2112
constexpr int kMaxSlabs = DINER_FMT_GRAD_MAX_SLABS;         // 1024
constexpr int kDefaultSlabs = 128;

// the layer pack (ops.pack_fmt_layer): the matrices TRANSPOSED, [k][out], then the vectors
constexpr int oWq = 0, oWk = 1024, oWv = 2048, oWo = 3072, oW1 = 4096, oW2 = 6144, oVec = 8192;
constexpr int vBq = 0, vBk = 32, vBv = 64, vBo = 96, vG1 = 128, vBe1 = 160, vB1 = 192, vB2 = 256, vG2 = 288, vBe2 = 320, kVec = 352;
static_assert(oVec + kVec == DINER_FMT_PACK_FLOATS, "pack layout");
static_assert(kHd == 4 && kD == 32 && kFF == 64 && kState == kHeads * (kHd * kHd + kHd), "the kernels are written for d_model 32, 8 heads, d_ff 64");
// a query slab: Wq Wo W1 W2 as (out, in), then bq bo g1 be1 b1 b2 g2 be2; a source slab: Wk Wv, then bk bv
constexpr int qWq = 0, qWo = 1024, qW1 = 2048, qW2 = 4096, qBq = 6144, qBo = 6176, qG1 = 6208, qBe1 = 6240, qB1 = 6272, qB2 = 6336, qG2 = 6368,
              qBe2 = 6400;
constexpr int sWk = 0, sWv = 1024, sBk = 2048, sBv = 2080;
static_assert(qBe2 + kD == kQSlab && sBv + kD == kSSlab, "slab layout");

struct FmtGradArgs {
  const float *x, *src, *pack, *state, *dy;
  float *d_x, *d_src, *d_state, *qslab, *sslab;
  double* partials;
  size_t carry;   // floats from a slab element to its carry: the size of the side's slab block
  int L, R, S, tiles, tiles_per_image, per, want_state, want_params, accumulate;
};

__device__ __forceinline__ float elu1(float v) { return (v > 0.0f ? v : expm1f(v)) + 1.0f; }
// elu'(v) from E = elu(v) + 1: v > 0 exactly where E > 1 (or E rounds to 1, where both forms give 1), otherwise exp(v) = E
__device__ __forceinline__ float elu1_slope(float e) { return e > 1.0f ? 1.0f : e; }

// acc[j] = bias[j] + sum_k col[k] Wt[k][j], one fmaf chain an output, k ascending: fmt.hip's token_gemm on this file's column stride
template <int NOUT, int NIN>
__device__ __forceinline__ void token_gemm(const float* col, const float* Wt, const float* bias, float* acc) {
#pragma unroll
  for (int j = 0; j < NOUT; ++j) acc[j] = bias[j];
#pragma unroll 2
  for (int k = 0; k < NIN; ++k) {
    const float xv = col[k * kLd];
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

// col[k] = sum_j g[j] Wt[k][j]: dX = dY W on the same [k][out] layout.  Four chains (j mod 4), each j ascending, added as (0 + 1) + (2 + 3).
template <int NOUT, int NIN>
__device__ __forceinline__ void token_gemm_back(const float* g, const float* Wt, float* col) {
#pragma unroll 2
  for (int k = 0; k < NIN; ++k) {
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
    for (int j = 0; j < NOUT; j += 4) {
      const v4f w = *reinterpret_cast<const v4f*>(&Wt[k * NOUT + j]);
      s0 = fmaf(g[j], w[0], s0);
      s1 = fmaf(g[j + 1], w[1], s1);
      s2 = fmaf(g[j + 2], w[2], s2);
      s3 = fmaf(g[j + 3], w[3], s3);
    }
    col[k * kLd] = (s0 + s1) + (s2 + s3);
  }
}

// torch's LayerNorm over the 32 channels as fmt.hip's layer_norm; v becomes the normalised value (before the affine), *rstd its scale
__device__ __forceinline__ void layer_norm_hat(float* v, float* rstd) {
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
  *rstd = 1.0f / sqrtf(q * (1.0f / kD) + 1e-5f);
#pragma unroll
  for (int j = 0; j < kD; ++j) v[j] = (v[j] - mean) * *rstd;
}

// g: the gradient at the LayerNorm's output -> at its input; hat, rstd from layer_norm_hat
__device__ __forceinline__ void layer_norm_back(float* g, const float* hat, float rstd, const float* gamma) {
  float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    g[j] *= gamma[j];
    m1 += g[j];
    m2 = fmaf(g[j], hat[j], m2);
  }
  m1 *= 1.0f / kD;
  m2 *= 1.0f / kD;
#pragma unroll
  for (int j = 0; j < kD; ++j) g[j] = rstd * ((g[j] - m1) - hat[j] * m2);
}

// (hi, lo) += p without losing the bits that do not fit hi: Knuth's two-sum; hi + lo carries a slab's tiles to about 2^-46
__device__ __forceinline__ void carry_add(float* hi, float* lo, float p, bool first) {
  if (first) {
    *hi = p;
    *lo = 0.0f;
    return;
  }
  const float h = *hi, s = h + p, bb = s - h;
  *lo += (h - (s - bb)) + (p - bb);
  *hi = s;
}

// The tile's sum_t G[j][t] A[k][t], t ascending, one fmaf chain from 0 an element, added to the slab's (slab, carry) pair: NJ x NK sums over
// the 128 threads, a thread four k's by TJ j's.  carry sits kCarry floats behind the slab.
template <int NJ, int NK>
__device__ __forceinline__ void outer_sums(const float* G, const float* A, float* slab, size_t carry, bool first, int tid) {
  constexpr int KG = NK / 4, JG = kTok / KG, TJ = NJ / JG;
  static_assert(TJ * JG == NJ && TJ >= 1, "patch");
  const int k0 = 4 * (tid % KG), j0 = TJ * (tid / KG);
  v4f acc[TJ];
#pragma unroll
  for (int b = 0; b < TJ; ++b) acc[b] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int t = 0; t < kTok; t += 4) {
    v4f av[4], gv[TJ];
#pragma unroll
    for (int a = 0; a < 4; ++a) av[a] = *reinterpret_cast<const v4f*>(&A[(k0 + a) * kLd + t]);
#pragma unroll
    for (int b = 0; b < TJ; ++b) gv[b] = *reinterpret_cast<const v4f*>(&G[(j0 + b) * kLd + t]);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int b = 0; b < TJ; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[b][a] = fmaf(gv[b][tt], av[a][tt], acc[b][a]);
  }
#pragma unroll
  for (int b = 0; b < TJ; ++b)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float* at = &slab[(j0 + b) * NK + k0 + a];
      carry_add(at, at + carry, acc[b][a], first);
    }
}

// the tile's sum_t row[t], t ascending from 0, in double (one thread a row: 128 adds), added to the (*out, out[carry]) pair as a float and
// what the float leaves.  A float chain here measured up to 1.16 of the bar on a LayerNorm bias of 35 tokens; torch adds such a sum as a tree.
__device__ __forceinline__ void row_sum(const float* row, float* out, size_t carry, bool first) {
  double s = 0.0;
#pragma unroll 4
  for (int t = 0; t < kTok; t += 4) {
    const v4f v = *reinterpret_cast<const v4f*>(&row[t]);
    s += (double)v[0];
    s += (double)v[1];
    s += (double)v[2];
    s += (double)v[3];
  }
  const float hi = (float)s;
  carry_add(out, out + carry, hi, first);
  out[carry] += (float)(s - (double)hi);
}

__device__ __forceinline__ void load_token(const float* p, bool live, float* v) {
#pragma unroll
  for (int q = 0; q < kD / 4; ++q) {
    v4f t = (v4f){0.f, 0.f, 0.f, 0.f};
    if (live) t = *reinterpret_cast<const v4f*>(p + 4 * q);
    v[4 * q] = t[0]; v[4 * q + 1] = t[1]; v[4 * q + 2] = t[2]; v[4 * q + 3] = t[3];
  }
}

// LDS of k_fmt_grad_query, in floats: the doubles first
constexpr int lRed = 0, lWq = lRed + 2 * 2 * kState, lWo = lWq + kD * kD, lW1 = lWo + kD * kD, lW2 = lW1 + kD * kFF, lVs = lW2 + kFF * kD,
              lSt = lVs + kVec, lAs = lSt + kState, lGs = lAs + kFF * kLd, lQueryFloats = lGs + kFF * kLd;
constexpr size_t kQueryLdsBytes = (size_t)lQueryFloats * sizeof(float);
static_assert(kQueryLdsBytes <= 160 * 1024 && lWq % 4 == 0 && lVs % 4 == 0 && lAs % 4 == 0 && lGs % 4 == 0, "LDS layout");

__global__ __launch_bounds__(kTok) void k_fmt_grad_query(FmtGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  double* red = reinterpret_cast<double*>(lds + lRed);                   // [wave][160]
  float *Wq = lds + lWq, *Wo = lds + lWo, *W1 = lds + lW1, *W2 = lds + lW2, *Vs = lds + lVs, *St = lds + lSt, *As = lds + lAs, *Gs = lds + lGs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < kD * kD / 4; e += kTok) {
    reinterpret_cast<v4f*>(Wq)[e] = reinterpret_cast<const v4f*>(a.pack + oWq)[e];
    reinterpret_cast<v4f*>(Wo)[e] = reinterpret_cast<const v4f*>(a.pack + oWo)[e];
  }
  for (int e = tid; e < kD * kFF / 4; e += kTok) {
    reinterpret_cast<v4f*>(W1)[e] = reinterpret_cast<const v4f*>(a.pack + oW1)[e];
    reinterpret_cast<v4f*>(W2)[e] = reinterpret_cast<const v4f*>(a.pack + oW2)[e];
  }
  for (int e = tid; e < kVec; e += kTok) Vs[e] = a.pack[oVec + e];
  float* acol = As + tid;
  float* gcol = Gs + tid;
  float* slab = a.qslab + (size_t)blockIdx.x * kQSlab;
  const int tile0 = (int)blockIdx.x * a.per, tile1 = min(tile0 + a.per, a.tiles);
  const bool params = a.want_params != 0;

#pragma unroll 1
  for (int tile = tile0; tile < tile1; ++tile) {
    const bool first = tile == tile0;
    const size_t n = (size_t)(tile / a.tiles_per_image);
    const int l = (tile % a.tiles_per_image) * kTok + tid;
    const bool live = l < a.L;
    const size_t at = (n * a.L + (live ? l : 0)) * kD;
    __syncthreads();                                                     // the tile before is done with St (and the weights are in)
    for (int e = tid; e < kState; e += kTok) St[e] = a.state[(n % (size_t)a.R) * kState + e];
    float xin[kD];
    load_token(a.x + at, live, xin);
#pragma unroll
    for (int k = 0; k < kD; ++k) acol[k * kLd] = xin[k];
    __syncthreads();

    // ---- the forward again, k_fmt_layer's chains; kept: the two normalised vectors, and relu(hidden) in the As column
    float hat1[kD], hat2[kD], rstd1, rstd2;
    {
      float q[kD], t[kD];
      token_gemm<kD, kD>(acol, Wq, Vs + vBq, q);
#pragma unroll
      for (int j = 0; j < kD; ++j) q[j] = elu1(q[j]);
#pragma unroll
      for (int h = 0; h < kHeads; ++h) {
        float den = 0.0f;
#pragma unroll
        for (int d = 0; d < kHd; ++d) den = fmaf(q[h * kHd + d], St[kHeads * kHd * kHd + h * kHd + d], den);
        const float z = 1.0f / (den + 1e-6f);
#pragma unroll
        for (int m = 0; m < kHd; ++m) {
          float s = 0.0f;
#pragma unroll
          for (int d = 0; d < kHd; ++d) s = fmaf(q[h * kHd + d], St[(h * kHd + m) * kHd + d], s);
          acol[(h * kHd + m) * kLd] = s * z;
        }
      }
      token_gemm<kD, kD>(acol, Wo, Vs + vBo, t);
#pragma unroll
      for (int j = 0; j < kD; ++j) hat1[j] = xin[j] + t[j];
      layer_norm_hat(hat1, &rstd1);
      float x1[kD];
#pragma unroll
      for (int j = 0; j < kD; ++j) {
        x1[j] = fmaf(hat1[j], Vs[vG1 + j], Vs[vBe1 + j]);
        acol[j * kLd] = x1[j];
      }
      float hdn[kFF];
      token_gemm<kFF, kD>(acol, W1, Vs + vB1, hdn);
#pragma unroll
      for (int k = 0; k < kFF; ++k) acol[k * kLd] = fmaxf(hdn[k], 0.0f);
      token_gemm<kD, kFF>(acol, W2, Vs + vB2, t);
#pragma unroll
      for (int j = 0; j < kD; ++j) hat2[j] = x1[j] + t[j];
      layer_norm_hat(hat2, &rstd2);
    }

    // ---- LN2
    float g[kD];                                                         // the running gradient of the residual stream
    load_token(a.dy + at, live, g);                                      // a token beyond L has dy = 0: every sum below gets +-0 from it
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      gcol[j * kLd] = g[j];
      gcol[(kD + j) * kLd] = g[j] * hat2[j];
    }
    if (params) {
      __syncthreads();
      if (tid < 2 * kD) row_sum(Gs + tid * kLd, slab + (tid < kD ? qBe2 + tid : qG2 + tid - kD), a.carry, first);
      __syncthreads();
    }
    layer_norm_back(g, hat2, rstd2, Vs + vG2);

    // ---- linear2: As holds relu(hidden)
#pragma unroll
    for (int j = 0; j < kD; ++j) gcol[j * kLd] = g[j];
    if (params) {
      __syncthreads();
      outer_sums<kD, kFF>(Gs, As, slab + qW2, a.carry, first, tid);
      if (tid < kD) row_sum(Gs + tid * kLd, slab + qB2 + tid, a.carry, first);
      __syncthreads();
    }
    token_gemm_back<kD, kFF>(g, W2, gcol);
    // ---- the ReLU and linear1
    float dh[kFF];
#pragma unroll
    for (int k = 0; k < kFF; ++k) {
      dh[k] = acol[k * kLd] > 0.0f ? gcol[k * kLd] : 0.0f;
      gcol[k * kLd] = dh[k];
    }
#pragma unroll
    for (int j = 0; j < kD; ++j) acol[j * kLd] = fmaf(hat1[j], Vs[vG1 + j], Vs[vBe1 + j]);      // x1 again
    if (params) {
      __syncthreads();
      outer_sums<kFF, kD>(Gs, As, slab + qW1, a.carry, first, tid);
      if (tid < kFF) row_sum(Gs + tid * kLd, slab + qB1 + tid, a.carry, first);
      __syncthreads();
    }
    token_gemm_back<kFF, kD>(dh, W1, acol);
#pragma unroll
    for (int j = 0; j < kD; ++j) g[j] += acol[j * kLd];

    // ---- LN1
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      gcol[j * kLd] = g[j];
      gcol[(kD + j) * kLd] = g[j] * hat1[j];
    }
    if (params) {
      __syncthreads();
      if (tid < 2 * kD) row_sum(Gs + tid * kLd, slab + (tid < kD ? qBe1 + tid : qG1 + tid - kD), a.carry, first);
      __syncthreads();
    }
    layer_norm_back(g, hat1, rstd1, Vs + vG1);

    // ---- the attention again: Q, 1 / den and A
    load_token(a.x + at, live, xin);
#pragma unroll
    for (int k = 0; k < kD; ++k) acol[k * kLd] = xin[k];
    float q[kD], z[kHeads], av[kD];
    token_gemm<kD, kD>(acol, Wq, Vs + vBq, q);
#pragma unroll
    for (int j = 0; j < kD; ++j) q[j] = elu1(q[j]);
#pragma unroll
    for (int h = 0; h < kHeads; ++h) {
      float den = 0.0f;
#pragma unroll
      for (int d = 0; d < kHd; ++d) den = fmaf(q[h * kHd + d], St[kHeads * kHd * kHd + h * kHd + d], den);
      z[h] = 1.0f / (den + 1e-6f);
#pragma unroll
      for (int m = 0; m < kHd; ++m) {
        float s = 0.0f;
#pragma unroll
        for (int d = 0; d < kHd; ++d) s = fmaf(q[h * kHd + d], St[(h * kHd + m) * kHd + d], s);
        av[h * kHd + m] = s * z[h];
        acol[(h * kHd + m) * kLd] = av[h * kHd + m];
      }
    }
    // ---- the out projection
#pragma unroll
    for (int j = 0; j < kD; ++j) gcol[j * kLd] = g[j];
    if (params) {
      __syncthreads();
      outer_sums<kD, kD>(Gs, As, slab + qWo, a.carry, first, tid);
      if (tid < kD) row_sum(Gs + tid * kLd, slab + qBo + tid, a.carry, first);
      __syncthreads();
    }
    token_gemm_back<kD, kD>(g, Wo, acol);                               // dA
    // ---- the attention's query side
    float dq[kD];
#pragma unroll
    for (int h = 0; h < kHeads; ++h) {
      float da[kHd], sa = 0.0f;
#pragma unroll
      for (int m = 0; m < kHd; ++m) {
        da[m] = acol[(h * kHd + m) * kLd];
        sa = fmaf(da[m], av[h * kHd + m], sa);
        da[m] *= z[h];                                                   // d numerator
      }
      const float dden = -(sa * z[h]);
#pragma unroll
      for (int d = 0; d < kHd; ++d) {
        float s = dden * St[kHeads * kHd * kHd + h * kHd + d];
#pragma unroll
        for (int m = 0; m < kHd; ++m) s = fmaf(da[m], St[(h * kHd + m) * kHd + d], s);
        dq[h * kHd + d] = s * elu1_slope(q[h * kHd + d]);
      }
      if (a.want_state) {
#pragma unroll
        for (int i = 0; i < kHd * kHd + kHd; ++i) {
          const int d = i & 3, m = i >> 2;
          const double v = (double)(i < kHd * kHd ? da[m & 3] : dden) * (double)q[h * kHd + d];
          const double s = wave_sum_d(v);
          const int to = i < kHd * kHd ? h * kHd * kHd + i : kHeads * kHd * kHd + h * kHd + d;
          if (lane == 0) red[wave * kState + to] = s;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kD; ++k) {
      acol[k * kLd] = xin[k];
      gcol[k * kLd] = dq[k];
    }
    if (params || a.want_state) {
      __syncthreads();
      if (params) {
        outer_sums<kD, kD>(Gs, As, slab + qWq, a.carry, first, tid);
        if (tid < kD) row_sum(Gs + tid * kLd, slab + qBq + tid, a.carry, first);
      }
      if (a.want_state) {
        for (int e = tid; e < kState; e += kTok) a.partials[(size_t)tile * kState + e] = red[e] + red[kState + e];
      }
      __syncthreads();
    }
    if (a.d_x) {
      token_gemm_back<kD, kD>(dq, Wq, acol);
      if (live) {
#pragma unroll
        for (int q4 = 0; q4 < kD / 4; ++q4) {
          v4f o;
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = g[4 * q4 + i] + acol[(4 * q4 + i) * kLd];
          *reinterpret_cast<v4f*>(a.d_x + at + 4 * q4) = o;
        }
      }
    }
  }
}

// the tiles' shares of a row in (image, tile) order over the images that read it, in double, rounded once
__global__ __launch_bounds__(192) void k_fmt_grad_state(const double* __restrict__ partials, float* __restrict__ d_state, int N, int R,
                                                         int tiles_per_image) {
  const int v = threadIdx.x, r = blockIdx.x;
  if (v >= kState) return;
  double s = 0.0;
  for (int n = r; n < N; n += R)
    for (int b = 0; b < tiles_per_image; ++b) s += partials[((size_t)n * tiles_per_image + b) * kState + v];
  d_state[(size_t)r * kState + v] = (float)s;
}

__global__ __launch_bounds__(kTok) void k_fmt_grad_source(FmtGradArgs a) {
  __shared__ __attribute__((aligned(16))) float Wk[kD * kD];
  __shared__ __attribute__((aligned(16))) float Wv[kD * kD];
  __shared__ float Bk[kD], Bv[kD], St[kState];
  __shared__ __attribute__((aligned(16))) float As[kD * kLd];
  __shared__ __attribute__((aligned(16))) float Gs[2 * kD * kLd];
  const int tid = threadIdx.x;
  for (int e = tid; e < kD * kD / 4; e += kTok) {
    reinterpret_cast<v4f*>(Wk)[e] = reinterpret_cast<const v4f*>(a.pack + oWk)[e];
    reinterpret_cast<v4f*>(Wv)[e] = reinterpret_cast<const v4f*>(a.pack + oWv)[e];
  }
  if (tid < kD) {
    Bk[tid] = a.pack[oVec + vBk + tid];
    Bv[tid] = a.pack[oVec + vBv + tid];
  }
  float* acol = As + tid;
  float* gcol = Gs + tid;
  float* slab = a.sslab + (size_t)blockIdx.x * kSSlab;
  const int tile0 = (int)blockIdx.x * a.per, tile1 = min(tile0 + a.per, a.tiles);
  const bool params = a.want_params != 0;

#pragma unroll 1
  for (int tile = tile0; tile < tile1; ++tile) {
    const bool first = tile == tile0;
    const size_t r = (size_t)(tile / a.tiles_per_image);
    const int s = (tile % a.tiles_per_image) * kTok + tid;
    const bool live = s < a.S;
    const size_t at = (r * a.S + (live ? s : 0)) * kD;
    __syncthreads();
    for (int e = tid; e < kState; e += kTok) St[e] = a.d_state[r * kState + e];
    float xin[kD];
    load_token(a.src + at, live, xin);
#pragma unroll
    for (int k = 0; k < kD; ++k) acol[k * kLd] = xin[k];
    __syncthreads();
    float kq[kD], vq[kD], dk[kD], dv[kD];
    token_gemm<kD, kD>(acol, Wk, Bk, kq);
    token_gemm<kD, kD>(acol, Wv, Bv, vq);
#pragma unroll
    for (int h = 0; h < kHeads; ++h) {
#pragma unroll
      for (int d = 0; d < kHd; ++d) {
        kq[h * kHd + d] = elu1(kq[h * kHd + d]);
        float t = St[kHeads * kHd * kHd + h * kHd + d];
#pragma unroll
        for (int m = 0; m < kHd; ++m) t = fmaf(St[(h * kHd + m) * kHd + d], vq[h * kHd + m], t);
        dk[h * kHd + d] = live ? t * elu1_slope(kq[h * kHd + d]) : 0.0f;            // a token beyond S adds +0
      }
#pragma unroll
      for (int m = 0; m < kHd; ++m) {
        float t = 0.0f;
#pragma unroll
        for (int d = 0; d < kHd; ++d) t = fmaf(St[(h * kHd + m) * kHd + d], kq[h * kHd + d], t);
        dv[h * kHd + m] = live ? t : 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      gcol[j * kLd] = dk[j];
      gcol[(kD + j) * kLd] = dv[j];
    }
    if (params) {
      __syncthreads();
      outer_sums<kD, kD>(Gs, As, slab + sWk, a.carry, first, tid);
      outer_sums<kD, kD>(Gs + kD * kLd, As, slab + sWv, a.carry, first, tid);
      if (tid < 2 * kD) row_sum(Gs + tid * kLd, slab + sBk + tid, a.carry, first);
      __syncthreads();
    }
    if (a.d_src) {
      token_gemm_back<kD, kD>(dk, Wk, acol);
      token_gemm_back<kD, kD>(dv, Wv, gcol);
      if (live) {
#pragma unroll
        for (int q4 = 0; q4 < kD / 4; ++q4) {
          v4f o;
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = acol[(4 * q4 + i) * kLd] + gcol[(4 * q4 + i) * kLd];
          v4f* to = reinterpret_cast<v4f*>(a.d_src + at + 4 * q4);
          if (a.accumulate) o = *to + o;                                 // the self layer: the query kernel's d_x plus the source path
          *to = o;
        }
      }
    }
  }
}

// one thread an element of the parameter block: its slabs (each with its carry) in slab order, in double, rounded once.  The block has the pack's order with the
// matrices as torch keeps them, (out, in): Wq Wk Wv Wo W1 W2, then bq bk bv bo g1 be1 b1 b2 g2 be2.
__global__ __launch_bounds__(256) void k_fmt_grad_finish(const float* __restrict__ qslab, const float* __restrict__ sslab, float* __restrict__ d_params,
                                                          int nq, int ns, size_t qcarry, size_t scarry) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= DINER_FMT_PACK_FLOATS) return;
  bool source = false;
  int at;
  if (e < oWk) at = qWq + e;
  else if (e < oWv) { source = true; at = sWk + (e - oWk); }
  else if (e < oWo) { source = true; at = sWv + (e - oWv); }
  else if (e < oW1) at = qWo + (e - oWo);
  else if (e < oW2) at = qW1 + (e - oW1);
  else if (e < oVec) at = qW2 + (e - oW2);
  else {
    const int v = e - oVec;
    if (v < vBk) at = qBq + v;
    else if (v < vBo) { source = true; at = sBk + (v - vBk); }          // bk, bv
    else at = qBo + (v - vBo);                                           // bo g1 be1 b1 b2 g2 be2, the slab's order
  }
  double sum = 0.0;
  if (source) {
    for (int s = 0; s < ns; ++s) sum += (double)sslab[(size_t)s * kSSlab + at] + (double)sslab[scarry + (size_t)s * kSSlab + at];
  } else {
    for (int s = 0; s < nq; ++s) sum += (double)qslab[(size_t)s * kQSlab + at] + (double)qslab[qcarry + (size_t)s * kQSlab + at];
  }
  d_params[e] = (float)sum;
}

struct FmtGradPlan {
  int tq, ts;             // tiles of an image on either side
  long long tiles_q, tiles_s;
  int slabs_q, slabs_s;   // the workspace's slab counts
};

bool grad_plan(int N, int L, int R, int S, int slabs, FmtGradPlan* p) {
  const int maxL = DINER_FMT_MAX_HW * DINER_FMT_MAX_HW;
  if (!(N >= 1 && N <= 65535 && R >= 1 && R <= N && N % R == 0 && L >= 1 && L <= maxL && S >= 1 && S <= maxL && slabs >= 0 && slabs <= kMaxSlabs))
    return false;
  p->tq = (L + kTok - 1) / kTok;
  p->ts = (S + kTok - 1) / kTok;
  p->tiles_q = (long long)N * p->tq;
  p->tiles_s = (long long)R * p->ts;
  if (p->tiles_q >= (1LL << 30) || p->tiles_s >= (1LL << 30)) return false;
  const long long want = slabs > 0 ? slabs : kDefaultSlabs;
  p->slabs_q = (int)(want < p->tiles_q ? want : p->tiles_q);
  p->slabs_s = (int)(want < p->tiles_s ? want : p->tiles_s);
  return true;
}

std::mutex g_attr_mu;
bool g_attr_set[64] = {};

int set_query_lds() {
  int dev = 0;
  DINER_HIP_OK(hipGetDevice(&dev));
  DINER_CHECK_ARG(dev >= 0 && dev < 64, "fmt_layer_grad: device index %d outside [0, 64)", dev);
  std::lock_guard<std::mutex> lock(g_attr_mu);
  if (!g_attr_set[dev]) {
    DINER_HIP_OK(hipFuncSetAttribute((const void*)k_fmt_grad_query, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQueryLdsBytes));
    g_attr_set[dev] = true;
  }
  return 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" size_t diner_fmt_layer_grad_workspace_floats(int N, int L, int R, int S, int slabs) {
  FmtGradPlan p;
  if (!grad_plan(N, L, R, S, slabs, &p)) return 0;
  return 2 * (size_t)p.tiles_q * kState + (size_t)R * kState + 2 * ((size_t)p.slabs_q * kQSlab + (size_t)p.slabs_s * kSSlab);
}

extern "C" int diner_fmt_layer_grad_f32(const float* x, const float* source, const float* pack, const float* state, const float* dy, int N, int L,
                                        int R, int S, float* d_x, float* d_source, float* d_params, float* workspace, int accumulate, int slabs,
                                        void* stream) {
  const int maxL = DINER_FMT_MAX_HW * DINER_FMT_MAX_HW;
  DINER_CHECK_ARG(N >= 1 && N <= 65535, "fmt_layer_grad: N = %d images (must be in [1, 65535])", N);
  DINER_CHECK_ARG(L >= 1 && L <= maxL && S >= 1 && S <= maxL, "fmt_layer_grad: L, S = %d, %d tokens (each must be in [1, %d])", L, S, maxL);
  DINER_CHECK_ARG(R >= 1 && R <= N && N % R == 0, "fmt_layer_grad: R = %d state rows (must divide N = %d: image n reads row n mod R)", R, N);
  DINER_CHECK_ARG(slabs >= 0 && slabs <= kMaxSlabs, "fmt_layer_grad: slabs = %d (0 for the default, or a count up to %d)", slabs, kMaxSlabs);
  FmtGradPlan p;
  DINER_CHECK_ARG(grad_plan(N, L, R, S, slabs, &p), "fmt_layer_grad: %d x %d and %d x %d tokens are too many tiles", N, L, R, S);
  DINER_CHECK_ARG(x && source && pack && state && dy, "fmt_layer_grad: null input pointer");
  DINER_CHECK_ARG(aligned16(x) && aligned16(source) && aligned16(pack) && aligned16(dy) && aligned16(d_x) && aligned16(d_source),
                  "fmt_layer_grad: the tokens, the pack and the token gradients must be 16-byte aligned");
  DINER_CHECK_ARG(((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(d_params)) & 3) == 0 && aligned16(workspace),
                  "fmt_layer_grad: state and d_params must be 4-byte, the workspace 16-byte aligned");
  DINER_CHECK_ARG(!accumulate || (source == x && N == R && L == S && !d_source),
                  "fmt_layer_grad: accumulate is the self layer: source must be x, R = N, S = L and d_source NULL (its gradient is added to d_x)");
  DINER_CHECK_ARG(!d_x || (d_x != x && d_x != source && d_x != dy), "fmt_layer_grad: d_x must not be one of the inputs");
  DINER_CHECK_ARG(!d_source || (d_source != x && d_source != source && d_source != dy && d_source != d_x),
                  "fmt_layer_grad: d_source must not be one of the inputs or d_x");
  const bool src_out = d_source || (accumulate && d_x), want_state = src_out || d_params;
  DINER_CHECK_ARG(!want_state || workspace,
                  "fmt_layer_grad: d_source, d_params and the self layer's d_x need the workspace (diner_fmt_layer_grad_workspace_floats)");
  if (!d_x && !want_state) return 0;
  int rc = set_query_lds();
  if (rc) return rc;

  FmtGradArgs a;
  a.x = x; a.src = source; a.pack = pack; a.state = state; a.dy = dy;
  a.d_x = d_x; a.d_src = nullptr; a.L = L; a.R = R; a.S = S;
  a.partials = reinterpret_cast<double*>(workspace);
  a.d_state = workspace ? workspace + 2 * (size_t)p.tiles_q * kState : nullptr;
  a.qslab = workspace ? a.d_state + (size_t)R * kState : nullptr;
  a.sslab = workspace ? a.qslab + 2 * (size_t)p.slabs_q * kQSlab : nullptr;       // each side: the slabs, then their carries
  a.want_state = want_state; a.want_params = d_params != nullptr; a.accumulate = 0;
  hipStream_t st = (hipStream_t)stream;

  a.tiles = (int)p.tiles_q; a.tiles_per_image = p.tq;
  a.per = (a.tiles + p.slabs_q - 1) / p.slabs_q;
  a.carry = (size_t)p.slabs_q * kQSlab;
  const int nq = (a.tiles + a.per - 1) / a.per;                          // no workgroup without a tile: nq <= slabs_q
  hipLaunchKernelGGL(k_fmt_grad_query, dim3((unsigned)nq), dim3(kTok), kQueryLdsBytes, st, a);
  DINER_LAUNCH_OK();
  if (!want_state) return 0;
  hipLaunchKernelGGL(k_fmt_grad_state, dim3((unsigned)R), dim3(192), 0, st, (const double*)a.partials, a.d_state, N, R, p.tq);
  DINER_LAUNCH_OK();
  a.tiles = (int)p.tiles_s; a.tiles_per_image = p.ts;
  a.per = (a.tiles + p.slabs_s - 1) / p.slabs_s;
  a.carry = (size_t)p.slabs_s * kSSlab;
  const int ns = (a.tiles + a.per - 1) / a.per;
  a.d_src = accumulate ? d_x : d_source;
  a.accumulate = accumulate != 0;
  hipLaunchKernelGGL(k_fmt_grad_source, dim3((unsigned)ns), dim3(kTok), 0, st, a);
  DINER_LAUNCH_OK();
  if (d_params) {
    hipLaunchKernelGGL(k_fmt_grad_finish, dim3((DINER_FMT_PACK_FLOATS + 255) / 256), dim3(256), 0, st, (const float*)a.qslab, (const float*)a.sslab,
                       d_params, nq, ns, (size_t)p.slabs_q * kQSlab, (size_t)p.slabs_s * kSSlab);
    DINER_LAUNCH_OK();
  }
  return 0;
}
