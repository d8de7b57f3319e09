// Alpha compositing along rays: one wavefront per ray, wave scan for the transmittance.
// Replaces the tail of NeRFRendererDGS.composite (reference nerf_renderer.py:299-301, :341-360).
#include "common.hpp"

namespace diner {

constexpr int kCompMaxPerLane = 4;       // K <= 256: the bounded entry
constexpr int kCompLongPerLane = 16;     // K <= 1024: the long entry above 256 samples

template <int kPerLane>
__global__ __launch_bounds__(256) void k_composite(const float4* __restrict__ field, const float* __restrict__ z,
                                                   const float* __restrict__ rays, int NR, int K, int per_lane,
                                                   int white_bkgd, float* __restrict__ rgb_out,
                                                   float* __restrict__ depth_out, float* __restrict__ weights_out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + wave;
  if (ray >= NR) return;                      // no block-level sync below: waves are independent
  const float far = rays[(size_t)ray * 8 + 7];
  const float* zr = z + (size_t)ray * K;
  const float4* fr = field + (size_t)ray * K;

  float alpha[kPerLane], zz[kPerLane];
  float4 f[kPerLane];
  float prod = 1.0f;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int k = lane * per_lane + j;
    alpha[j] = 0.0f; zz[j] = 0.0f; f[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < per_lane && k < K) {
      zz[j] = zr[k];
      const float znext = (k + 1 < K) ? zr[k + 1] : far;                    // :299-301
      const float delta = __fsub_rn(znext, zz[j]);
      f[j] = fr[k];
      const float sig = fmaxf(f[j].w, 0.0f);                                 // relu again (idempotent) :344
      alpha[j] = __fsub_rn(1.0f, expf(-__fmul_rn(delta, sig)));
      prod *= __fadd_rn(__fsub_rn(1.0f, alpha[j]), 1e-10f);                  // :348
    }
  }
  float incl = prod;                          // inclusive multiplicative scan over lanes
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const float up = __shfl_up(incl, o, kWave);
    if (lane >= o) incl *= up;
  }
  float T = __shfl_up(incl, 1, kWave);
  if (lane == 0) T = 1.0f;
  float r = 0.f, g = 0.f, b = 0.f, d = 0.f, wsum = 0.f;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int k = lane * per_lane + j;
    if (j < per_lane && k < K) {
      const float w = __fmul_rn(alpha[j], T);                                // :351
      T *= __fadd_rn(__fsub_rn(1.0f, alpha[j]), 1e-10f);
      r += w * f[j].x; g += w * f[j].y; b += w * f[j].z;                     // :355
      d += w * zz[j];                                                        // :356
      wsum += w;
      if (weights_out) weights_out[(size_t)ray * K + k] = w;
    }
  }
  r = wave_sum(r); g = wave_sum(g); b = wave_sum(b); d = wave_sum(d); wsum = wave_sum(wsum);
  if (lane == 0) {
    if (white_bkgd) {                                                        // :357-360
      const float bg = 1.0f - wsum;
      r += bg; g += bg; b += bg;
    }
    rgb_out[(size_t)ray * 3 + 0] = r;
    rgb_out[(size_t)ray * 3 + 1] = g;
    rgb_out[(size_t)ray * 3 + 2] = b;
    depth_out[ray] = d;
  }
}

// k_composite with the ray's opacity and depth spread as two more per-ray outputs (either may be null):
//   alpha = sum_k w_k -- the pix_alpha of nerf_renderer.py:359, which the reference uses for the white background and drops;
//   depth_var = max(0, sum_k w_k (z_k - depth)^2) around the unnormalised depth = sum_k w_k z_k of :356 -- the centred form, in a second
//   pass over the w and z the lane holds (sum w z^2 - depth^2 cancels); the sum is negative only where a weight is (a sample beyond `far`).
// rgb, depth and weights: the arithmetic of k_composite in its order, hence its bits.  The weights take the registers of the
// per-sample alphas once those are consumed, so the instance carries no more per-sample state than k_composite.
template <int kPerLane>
__global__ __launch_bounds__(256) void k_composite_aux(const float4* __restrict__ field, const float* __restrict__ z,
                                                       const float* __restrict__ rays, int NR, int K, int per_lane,
                                                       int white_bkgd, float* __restrict__ rgb_out,
                                                       float* __restrict__ depth_out, float* __restrict__ weights_out,
                                                       float* __restrict__ alpha_out, float* __restrict__ depth_var_out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + wave;
  if (ray >= NR) return;                      // no block-level sync below: waves are independent
  const float far = rays[(size_t)ray * 8 + 7];
  const float* zr = z + (size_t)ray * K;
  const float4* fr = field + (size_t)ray * K;

  float alpha[kPerLane], zz[kPerLane];        // alpha[j] becomes w_j in the compositing loop
  float4 f[kPerLane];
  float prod = 1.0f;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int k = lane * per_lane + j;
    alpha[j] = 0.0f; zz[j] = 0.0f; f[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < per_lane && k < K) {
      zz[j] = zr[k];
      const float znext = (k + 1 < K) ? zr[k + 1] : far;                    // :299-301
      const float delta = __fsub_rn(znext, zz[j]);
      f[j] = fr[k];
      const float sig = fmaxf(f[j].w, 0.0f);                                 // :344
      alpha[j] = __fsub_rn(1.0f, expf(-__fmul_rn(delta, sig)));
      prod *= __fadd_rn(__fsub_rn(1.0f, alpha[j]), 1e-10f);                  // :348
    }
  }
  float incl = prod;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const float up = __shfl_up(incl, o, kWave);
    if (lane >= o) incl *= up;
  }
  float T = __shfl_up(incl, 1, kWave);
  if (lane == 0) T = 1.0f;
  float r = 0.f, g = 0.f, b = 0.f, d = 0.f, wsum = 0.f;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int k = lane * per_lane + j;
    if (j < per_lane && k < K) {
      const float w = __fmul_rn(alpha[j], T);                                // :351
      T *= __fadd_rn(__fsub_rn(1.0f, alpha[j]), 1e-10f);
      r += w * f[j].x; g += w * f[j].y; b += w * f[j].z;                     // :355
      d += w * zz[j];                                                        // :356
      wsum += w;
      if (weights_out) weights_out[(size_t)ray * K + k] = w;
      alpha[j] = w;
    }
  }
  r = wave_sum(r); g = wave_sum(g); b = wave_sum(b); d = wave_sum(d); wsum = wave_sum(wsum);
  float var = 0.f;                            // every lane holds the ray's depth after the butterfly
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const float dz = zz[j] - d;
    var += alpha[j] * (dz * dz);              // empty slots kept alpha = 0
  }
  var = wave_sum(var);
  if (lane == 0) {
    if (white_bkgd) {                                                        // :357-360
      const float bg = 1.0f - wsum;
      r += bg; g += bg; b += bg;
    }
    rgb_out[(size_t)ray * 3 + 0] = r;
    rgb_out[(size_t)ray * 3 + 1] = g;
    rgb_out[(size_t)ray * 3 + 2] = b;
    depth_out[ray] = d;
    if (alpha_out) alpha_out[ray] = wsum;                                    // :359
    if (depth_var_out) depth_var_out[ray] = var < 0.0f ? 0.0f : var;
  }
}

}  // namespace diner

using namespace diner;

extern "C" int diner_composite_f32(const float* field, const float* z, const float* rays, int NR, int K,
                                   int white_bkgd, float* rgb_out, float* depth_out, float* weights_out,
                                   void* stream) {
  DINER_CHECK_ARG(field && z && rays && rgb_out && depth_out, "composite: null pointer argument");
  DINER_CHECK_ARG(NR > 0 && K > 0 && K <= kWave * kCompMaxPerLane, "composite: bad sizes NR=%d K=%d (K <= %d)", NR, K,
                  kWave * kCompMaxPerLane);
  const int per_lane = (K + kWave - 1) / kWave;
  hipLaunchKernelGGL(k_composite<kCompMaxPerLane>, dim3((NR + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float4*)field, z, rays,
                     NR, K, per_lane, white_bkgd, rgb_out, depth_out, weights_out);
  DINER_LAUNCH_OK();
  return 0;
}

// long entry: today's instance wherever it fits (K <= 256), 16 samples per lane above
extern "C" int diner_composite_long_f32(const float* field, const float* z, const float* rays, int NR, int K,
                                        int white_bkgd, float* rgb_out, float* depth_out, float* weights_out,
                                        void* stream) {
  DINER_CHECK_ARG(field && z && rays && rgb_out && depth_out, "composite_long: null pointer argument");
  DINER_CHECK_ARG(NR > 0 && K > 0 && K <= kWave * kCompLongPerLane, "composite_long: bad sizes NR=%d K=%d (K <= %d)", NR, K,
                  kWave * kCompLongPerLane);
  if (K <= kWave * kCompMaxPerLane)
    return diner_composite_f32(field, z, rays, NR, K, white_bkgd, rgb_out, depth_out, weights_out, stream);
  const int per_lane = (K + kWave - 1) / kWave;
  hipLaunchKernelGGL(k_composite<kCompLongPerLane>, dim3((NR + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)field, z, rays, NR, K, per_lane, white_bkgd, rgb_out, depth_out, weights_out);
  DINER_LAUNCH_OK();
  return 0;
}

// opacity and depth spread beside colour and depth (nerf_renderer.py:359): whole range K <= 1024, per-lane width as the long entry
extern "C" int diner_composite_aux_f32(const float* field, const float* z, const float* rays, int NR, int K, int white_bkgd,
                                       float* rgb_out, float* depth_out, float* weights_out, float* alpha_out,
                                       float* depth_var_out, void* stream) {
  DINER_CHECK_ARG(field && z && rays && rgb_out && depth_out, "composite_aux: null pointer argument");
  DINER_CHECK_ARG(NR > 0 && K > 0 && K <= kWave * kCompLongPerLane, "composite_aux: bad sizes NR=%d K=%d (K <= %d)", NR, K,
                  kWave * kCompLongPerLane);
  const int per_lane = (K + kWave - 1) / kWave;
  if (K <= kWave * kCompMaxPerLane)
    hipLaunchKernelGGL(k_composite_aux<kCompMaxPerLane>, dim3((NR + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float4*)field, z,
                       rays, NR, K, per_lane, white_bkgd, rgb_out, depth_out, weights_out, alpha_out, depth_var_out);
  else
    hipLaunchKernelGGL(k_composite_aux<kCompLongPerLane>, dim3((NR + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float4*)field, z,
                       rays, NR, K, per_lane, white_bkgd, rgb_out, depth_out, weights_out, alpha_out, depth_var_out);
  DINER_LAUNCH_OK();
  return 0;
}
