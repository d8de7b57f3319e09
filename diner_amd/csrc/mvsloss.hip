// The fine-tuning objective of the multi-view depth estimator and its depth scores (TransMVSNet's entropy_loss / focal_loss_bld /
// trans_mvsnet_loss, models/module.py:490-587, and Thres_metrics / AbsDepthError_metrics, utils.py:240-274), with the gradient.
//   k_mvs_stage_loss<FROM_PROB>       one stage's forward: per pixel the softmax statistics, the ground-truth plane, the cross entropy, the
//                                     winner-take-all depth and its errors; per workgroup partial sums in double
//   k_mvs_loss_finish                 the per-image sums in a fixed order -> the stage's scalars and the backward's per-image factors
//   k_mvs_stage_loss_grad<FROM_PROB>  d(upstream weight 2 entropy) / d(cost | prob) as one dense volume
//   k_depth_scores, k_depth_scores_finish   the per-image and batch-mean depth scores
// One thread owns one pixel and walks its D planes, as k_mvs_select_depth does (mvs.hip), with the same expf / logf chain, so depth and
// confidence have that kernel's bits.  No atomics: a workgroup belongs to one image and writes its partial sums to its own slot; the
// finish kernels add an image's slots in an order the shape alone fixes (lane l takes slots l, l + 64, ..., then the xor tree), so two
// runs give the same bits and an image's sums do not depend on its place in the batch.  Layouts and limits: include/diner_hip.h.
#include "common.hpp"

namespace diner {

namespace {

constexpr int kLossThreads = 256;
constexpr int kLossSlots = DINER_MVS_LOSS_SLOTS;             // doubles per workgroup / per image
constexpr int kMaxThr = DINER_MVS_LOSS_MAX_THRESHOLDS;
// slot layout of the stage loss: valid, sum ce, sum smooth-L1, sum |err|, sum |err| / unit, counts of |err| / unit < threshold t
enum { S_VALID = 0, S_CE = 1, S_SL1 = 2, S_ABS = 3, S_SCALED = 4, S_CNT = 5 };
// slot layout of the depth scores: valid, sum |err|, sum |err| inside the band, count inside the band, counts of |err| > threshold t
enum { Q_VALID = 0, Q_ABS = 1, Q_BAND = 2, Q_NBAND = 3, Q_CNT = 4 };

struct Thresholds {
  double t[kMaxThr];
  int n;
};

struct StageArgs {
  const float* vol;        // (B,D,H,W): the cost, or with FROM_PROB the probability volume
  const float* init;       // (B,D,H,W) addend of the cost, or null
  const float* hyp;        // (B,D,H,W)
  const float* gt;         // (B,H,W)
  const float* mask;       // (B,H,W), valid where > 0.5
  const double* unit;      // (B) the scores' error unit per image, or null: no scores
  float* depth;            // (B,H,W)
  float* conf;             // (B,H,W)
  float* rec;              // (B,H,W,4): g (as int bits), prob[g], max, log-sum; or null
  double* part;            // (B, blocks_per_image, kLossSlots)
  int D, HW, blocks_per_image;
};

template <bool FROM_PROB>
__device__ __forceinline__ float vol_at(const StageArgs& a, size_t idx) {
  float c = a.vol[idx];
  if (!FROM_PROB && a.init != nullptr) c = __fadd_rn(c, a.init[idx]);
  return c;
}

template <bool FROM_PROB>
__global__ void __launch_bounds__(kLossThreads) k_mvs_stage_loss(StageArgs a, Thresholds thr) {
  __shared__ double red[kLossThreads / 64];
  const int b = blockIdx.x / a.blocks_per_image, blk = blockIdx.x - b * a.blocks_per_image;
  const int pix = blk * kLossThreads + threadIdx.x;
  const int D = a.D, HW = a.HW;
  const bool live = pix < HW;
  double s_valid = 0.0, s_ce = 0.0, s_sl1 = 0.0, s_abs = 0.0, s_scaled = 0.0;
  int cnt[kMaxThr];
#pragma unroll
  for (int t = 0; t < kMaxThr; ++t) cnt[t] = 0;
  if (live) {
    const size_t base = (size_t)b * D * HW + pix;
    const size_t p2 = (size_t)b * HW + pix;
    const bool valid = a.mask[p2] > 0.5f;
    const float gt = a.gt[p2];
    // the ground-truth plane: the first index of min_d |hyp_d - gt|; 0 where the mask is off (the reference multiplies the index by it)
    int g = 0;
    if (valid) {
      float bestd = INFINITY;
      for (int d = 0; d < D; ++d) {
        const float e = fabsf(__fsub_rn(a.hyp[base + (size_t)d * HW], gt));
        if (e < bestd) { bestd = e; g = d; }
      }
    }
    float m = 0.0f, lse = 0.0f;
    if (!FROM_PROB) {
      m = -INFINITY;
      for (int d = 0; d < D; ++d) m = fmaxf(m, vol_at<FROM_PROB>(a, base + (size_t)d * HW));
      float sum = 0.0f;
      for (int d = 0; d < D; ++d) sum = __fadd_rn(sum, expf(__fsub_rn(vol_at<FROM_PROB>(a, base + (size_t)d * HW), m)));
      lse = logf(sum);
    }
    float best = -1.0f, pg = 0.0f;
    int arg = 0;
    for (int d = 0; d < D; ++d) {
      const float c = vol_at<FROM_PROB>(a, base + (size_t)d * HW);
      const float pr = FROM_PROB ? c : expf(__fsub_rn(__fsub_rn(c, m), lse));
      if (pr > best) { best = pr; arg = d; }    // strict: the first index of the maximum
      if (d == g) pg = pr;
    }
    const float dep = a.hyp[base + (size_t)arg * HW];
    a.depth[p2] = dep;
    a.conf[p2] = best;
    if (a.rec != nullptr) {
      float4 r;
      r.x = __int_as_float(g); r.y = pg; r.z = m; r.w = lse;
      reinterpret_cast<float4*>(a.rec)[p2] = r;
    }
    if (valid) {                                 // an unmasked pixel adds nothing, whatever gt holds
      s_valid = 1.0;
      s_ce = -(double)logf(__fadd_rn(pg, 1e-6f));
      const double e = fabs((double)dep - (double)gt);
      s_abs = e;
      s_sl1 = e < 1.0 ? 0.5 * e * e : e - 0.5;
      if (a.unit != nullptr) {
        const double sc = e / a.unit[b];
        s_scaled = sc;
#pragma unroll
        for (int t = 0; t < kMaxThr; ++t) cnt[t] = (t < thr.n && sc < thr.t[t]) ? 1 : 0;
      }
    }
  }
  double* slot = a.part + (size_t)blockIdx.x * kLossSlots;
  const double v0 = block_sum_d<kLossThreads / 64>(s_valid, red);
  const double v1 = block_sum_d<kLossThreads / 64>(s_ce, red);
  const double v2 = block_sum_d<kLossThreads / 64>(s_sl1, red);
  const double v3 = block_sum_d<kLossThreads / 64>(s_abs, red);
  const double v4 = block_sum_d<kLossThreads / 64>(s_scaled, red);
  if (threadIdx.x == 0) { slot[S_VALID] = v0; slot[S_CE] = v1; slot[S_SL1] = v2; slot[S_ABS] = v3; slot[S_SCALED] = v4; }
#pragma unroll
  for (int t = 0; t < kMaxThr; ++t) {
    const double c = block_sum_d<kLossThreads / 64>((double)cnt[t], red);
    if (threadIdx.x == 0) slot[S_CNT + t] = c;
  }
}

// one wave: the sum of slot s over an image's n workgroups, lane l adding workgroups l, l + 64, ... in order, then the xor tree
__device__ __forceinline__ double image_sum(const double* part, int n, int s) {
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += 64) v += part[(size_t)k * kLossSlots + s];
  return wave_sum_d(v);
}

// One wave.  scalars (float, DINER_MVS_LOSS_SCALARS): weight 2 entropy, 2 entropy, depth_loss, mean |err|, mean |err| / unit, then the
// share of valid pixels under each threshold.  fac (B, double): 1 / (B (float32(valid_b) + 1e-6)), the sum rounded to float32.  sums (B, kLossSlots): the per-image sums.
__global__ void __launch_bounds__(64) k_mvs_loss_finish(const double* __restrict__ part, int B, int blocks_per_image, int n_thr, double weight,
                                                        float* __restrict__ scalars, double* __restrict__ fac, double* __restrict__ sums) {
  double ent = 0.0, tot[kLossSlots];
#pragma unroll
  for (int s = 0; s < kLossSlots; ++s) tot[s] = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* p = part + (size_t)b * blocks_per_image * kLossSlots;
    double v[kLossSlots];
#pragma unroll
    for (int s = 0; s < kLossSlots; ++s) {
      v[s] = s < S_CNT + kMaxThr ? image_sum(p, blocks_per_image, s) : 0.0;      // the slots beyond are never written
      tot[s] += v[s];
    }
    const double denom = (double)__fadd_rn((float)v[S_VALID], 1e-6f);      // the reference's float32 valid_pixel_num + 1e-6
    ent += v[S_CE] / denom;                      // 0 for an image without a valid pixel
    if (threadIdx.x == 0) {
      fac[b] = 1.0 / ((double)B * denom);
#pragma unroll
      for (int s = 0; s < kLossSlots; ++s) sums[(size_t)b * kLossSlots + s] = v[s];
    }
  }
  if (threadIdx.x == 0) {
    ent /= (double)B;
    const double n = tot[S_VALID];               // 0 / 0 = NaN when nothing is valid, as the mean of an empty selection
    scalars[0] = (float)(weight * 2.0 * ent);
    scalars[1] = (float)(2.0 * ent);
    scalars[2] = (float)(tot[S_SL1] / n);
    scalars[3] = (float)(tot[S_ABS] / n);
    scalars[4] = (float)(tot[S_SCALED] / n);
#pragma unroll
    for (int t = 0; t < kMaxThr; ++t) scalars[5 + t] = t < n_thr ? (float)(tot[S_CNT + t] / n) : 0.0f;
  }
}

struct GradArgs {
  const float* vol;
  const float* init;
  const float* mask;
  const float* rec;
  const double* fac;       // (B)
  const float* upstream;   // device scalar
  float* grad;             // (B,D,H,W)
  double weight;
  int D, HW, blocks_per_image;
};

template <bool FROM_PROB>
__global__ void __launch_bounds__(kLossThreads) k_mvs_stage_loss_grad(GradArgs a) {
  const int b = blockIdx.x / a.blocks_per_image, blk = blockIdx.x - b * a.blocks_per_image;
  const int pix = blk * kLossThreads + threadIdx.x;
  if (pix >= a.HW) return;
  const int D = a.D, HW = a.HW;
  const size_t base = (size_t)b * D * HW + pix;
  const size_t p2 = (size_t)b * HW + pix;
  float* o = a.grad + base;
  if (!(a.mask[p2] > 0.5f)) {                    // zeros, not NaN
    for (int d = 0; d < D; ++d) o[(size_t)d * HW] = 0.0f;
    return;
  }
  const float4 r = reinterpret_cast<const float4*>(a.rec)[p2];
  const int g = __float_as_int(r.x);
  const float pg = r.y, m = r.z, lse = r.w;
  const double G = -(double)a.upstream[0] * a.weight * 2.0 * a.fac[b] / (double)__fadd_rn(pg, 1e-6f);
  if (FROM_PROB) {
    for (int d = 0; d < D; ++d) o[(size_t)d * HW] = d == g ? (float)G : 0.0f;
    return;
  }
  const double Gp = G * (double)pg;
  for (int d = 0; d < D; ++d) {
    float c = a.vol[base + (size_t)d * HW];
    if (a.init != nullptr) c = __fadd_rn(c, a.init[base + (size_t)d * HW]);
    const float pr = expf(__fsub_rn(__fsub_rn(c, m), lse));
    o[(size_t)d * HW] = (float)(Gp * ((d == g ? 1.0 : 0.0) - (double)pr));
  }
}

__global__ void __launch_bounds__(kLossThreads) k_depth_scores(const float* __restrict__ est, const float* __restrict__ gt,
                                                               const float* __restrict__ mask, double* __restrict__ part, int HW,
                                                               int blocks_per_image, int has_band, double lo, double hi, Thresholds thr) {
  __shared__ double red[kLossThreads / 64];
  const int b = blockIdx.x / blocks_per_image, blk = blockIdx.x - b * blocks_per_image;
  const int pix = blk * kLossThreads + threadIdx.x;
  double s_valid = 0.0, s_abs = 0.0, s_band = 0.0, s_nband = 0.0;
  int cnt[kMaxThr];
#pragma unroll
  for (int t = 0; t < kMaxThr; ++t) cnt[t] = 0;
  if (pix < HW) {
    const size_t p2 = (size_t)b * HW + pix;
    if (mask[p2] > 0.5f) {
      const double e = fabs((double)est[p2] - (double)gt[p2]);
      s_valid = 1.0;
      s_abs = e;
      if (has_band && e >= lo && e <= hi) { s_band = e; s_nband = 1.0; }
#pragma unroll
      for (int t = 0; t < kMaxThr; ++t) cnt[t] = (t < thr.n && e > thr.t[t]) ? 1 : 0;
    }
  }
  double* slot = part + (size_t)blockIdx.x * kLossSlots;
  const double v0 = block_sum_d<kLossThreads / 64>(s_valid, red);
  const double v1 = block_sum_d<kLossThreads / 64>(s_abs, red);
  const double v2 = block_sum_d<kLossThreads / 64>(s_band, red);
  const double v3 = block_sum_d<kLossThreads / 64>(s_nband, red);
  if (threadIdx.x == 0) { slot[Q_VALID] = v0; slot[Q_ABS] = v1; slot[Q_BAND] = v2; slot[Q_NBAND] = v3; }
#pragma unroll
  for (int t = 0; t < kMaxThr; ++t) {
    const double c = block_sum_d<kLossThreads / 64>((double)cnt[t], red);
    if (threadIdx.x == 0) slot[Q_CNT + t] = c;
  }
}

// One wave.  per_image (B, DINER_DEPTH_SCORES): mean |err|, mean |err| inside the band (0 when the band is empty), the share of errors
// above each threshold; batch (DINER_DEPTH_SCORES): the mean of the per-image values over the batch, images in order.
__global__ void __launch_bounds__(64) k_depth_scores_finish(const double* __restrict__ part, int B, int blocks_per_image, int n_thr,
                                                            float* __restrict__ per_image, float* __restrict__ batch) {
  double acc[2 + kMaxThr];
#pragma unroll
  for (int s = 0; s < 2 + kMaxThr; ++s) acc[s] = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* p = part + (size_t)b * blocks_per_image * kLossSlots;
    const double n = image_sum(p, blocks_per_image, Q_VALID);
    const double nb = image_sum(p, blocks_per_image, Q_NBAND);
    double v[2 + kMaxThr];
    v[0] = image_sum(p, blocks_per_image, Q_ABS) / n;            // NaN without a valid pixel: the mean of an empty selection
    const double band = image_sum(p, blocks_per_image, Q_BAND);
    v[1] = nb > 0.0 ? band / nb : 0.0;
#pragma unroll
    for (int t = 0; t < kMaxThr; ++t) {
      const double c = image_sum(p, blocks_per_image, Q_CNT + t);
      v[2 + t] = t < n_thr ? c / n : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 2 + kMaxThr; ++s) {
      acc[s] += v[s];
      if (threadIdx.x == 0) per_image[(size_t)b * (2 + kMaxThr) + s] = (float)v[s];
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < 2 + kMaxThr; ++s) batch[s] = (float)(acc[s] / (double)B);
  }
}

int loss_plan(const char* who, int B, int D, int H, int W, int* blocks_per_image, int* grid) {
  DINER_CHECK_ARG(B >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: B = %d, D = %d, H = %d, W = %d must be >= 1", who, B, D, H, W);
  DINER_CHECK_ARG((long long)B * D * H * W < (1ll << 31), "%s: B D H W = %lld must stay below 2^31", who, (long long)B * D * H * W);
  *blocks_per_image = (H * W + kLossThreads - 1) / kLossThreads;
  *grid = *blocks_per_image * B;                 // <= B H W < 2^31
  return 0;
}

int fill_thresholds(const char* who, const double* thresholds, int n, Thresholds* out) {
  DINER_CHECK_ARG(n >= 0 && n <= kMaxThr, "%s: %d thresholds outside [0, %d]", who, n, kMaxThr);
  DINER_CHECK_ARG(n == 0 || thresholds != nullptr, "%s: null thresholds", who);
  out->n = n;
  for (int t = 0; t < kMaxThr; ++t) out->t[t] = t < n ? thresholds[t] : 0.0;
  return 0;
}

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" size_t diner_mvs_loss_partial_doubles(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return 0;
  return (size_t)B * ((H * W + kLossThreads - 1) / kLossThreads) * kLossSlots;
}

extern "C" int diner_mvs_stage_loss_f32(const float* cost, const float* init, const float* prob, const float* hypotheses, const float* gt,
                                        const float* mask, const double* unit, const double* thresholds, int n_thresholds, float* depth,
                                        float* confidence, float* record, double* partials, int B, int D, int H, int W, void* stream) {
  DINER_CHECK_ARG((cost != nullptr) != (prob != nullptr), "mvs_stage_loss: give either the cost or the probability volume");
  DINER_CHECK_ARG(prob == nullptr || init == nullptr, "mvs_stage_loss: the addend belongs to the cost, not to a probability volume");
  DINER_CHECK_ARG(hypotheses && gt && mask && depth && confidence && partials, "mvs_stage_loss: null pointer");
  DINER_CHECK_ARG(record == nullptr || (uintptr_t)record % 16 == 0, "mvs_stage_loss: the record must be 16-byte aligned");
  int bpi = 0, grid = 0;
  const int rc = loss_plan("mvs_stage_loss", B, D, H, W, &bpi, &grid);
  if (rc) return rc;
  Thresholds thr;
  const int rt = fill_thresholds("mvs_stage_loss", thresholds, unit ? n_thresholds : 0, &thr);
  if (rt) return rt;
  StageArgs a;
  a.vol = cost ? cost : prob; a.init = init; a.hyp = hypotheses; a.gt = gt; a.mask = mask; a.unit = unit;
  a.depth = depth; a.conf = confidence; a.rec = record; a.part = partials;
  a.D = D; a.HW = H * W; a.blocks_per_image = bpi;
  if (cost)
    hipLaunchKernelGGL(k_mvs_stage_loss<false>, dim3(grid), dim3(kLossThreads), 0, (hipStream_t)stream, a, thr);
  else
    hipLaunchKernelGGL(k_mvs_stage_loss<true>, dim3(grid), dim3(kLossThreads), 0, (hipStream_t)stream, a, thr);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_mvs_loss_finish_f32(const double* partials, int B, int H, int W, int n_thresholds, double weight, float* scalars,
                                         double* factors, double* sums, void* stream) {
  DINER_CHECK_ARG(partials && scalars && factors && sums, "mvs_loss_finish: null pointer");
  DINER_CHECK_ARG(n_thresholds >= 0 && n_thresholds <= kMaxThr, "mvs_loss_finish: %d thresholds outside [0, %d]", n_thresholds, kMaxThr);
  int bpi = 0, grid = 0;
  const int rc = loss_plan("mvs_loss_finish", B, 1, H, W, &bpi, &grid);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mvs_loss_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, B, bpi, n_thresholds, weight, scalars, factors,
                     sums);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_mvs_stage_loss_grad_f32(const float* cost, const float* init, int from_prob, const float* mask, const float* record,
                                             const double* factors, const float* upstream, double weight, float* grad, int B, int D, int H,
                                             int W, void* stream) {
  DINER_CHECK_ARG(mask && record && factors && upstream && grad, "mvs_stage_loss_grad: null pointer");
  DINER_CHECK_ARG(from_prob || cost, "mvs_stage_loss_grad: the gradient with respect to the cost needs the cost");
  DINER_CHECK_ARG(!from_prob || init == nullptr, "mvs_stage_loss_grad: the addend belongs to the cost, not to a probability volume");
  DINER_CHECK_ARG((uintptr_t)record % 16 == 0, "mvs_stage_loss_grad: the record must be 16-byte aligned");
  int bpi = 0, grid = 0;
  const int rc = loss_plan("mvs_stage_loss_grad", B, D, H, W, &bpi, &grid);
  if (rc) return rc;
  GradArgs a;
  a.vol = cost; a.init = init; a.mask = mask; a.rec = record; a.fac = factors; a.upstream = upstream; a.grad = grad; a.weight = weight;
  a.D = D; a.HW = H * W; a.blocks_per_image = bpi;
  if (from_prob)
    hipLaunchKernelGGL(k_mvs_stage_loss_grad<true>, dim3(grid), dim3(kLossThreads), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_mvs_stage_loss_grad<false>, dim3(grid), dim3(kLossThreads), 0, (hipStream_t)stream, a);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_depth_scores_f32(const float* est, const float* gt, const float* mask, int B, int H, int W, const double* thresholds,
                                      int n_thresholds, int has_band, double band_lo, double band_hi, double* partials, float* per_image,
                                      float* batch, void* stream) {
  DINER_CHECK_ARG(est && gt && mask && partials && per_image && batch, "depth_scores: null pointer");
  int bpi = 0, grid = 0;
  const int rc = loss_plan("depth_scores", B, 1, H, W, &bpi, &grid);
  if (rc) return rc;
  Thresholds thr;
  const int rt = fill_thresholds("depth_scores", thresholds, n_thresholds, &thr);
  if (rt) return rt;
  hipLaunchKernelGGL(k_depth_scores, dim3(grid), dim3(kLossThreads), 0, (hipStream_t)stream, est, gt, mask, partials, H * W, bpi,
                     has_band ? 1 : 0, band_lo, band_hi, thr);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_depth_scores_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, B, bpi, n_thresholds, per_image,
                     batch);
  DINER_LAUNCH_OK();
  return 0;
}
