// Depth-guided ray sampler + stratified fill: one wavefront (64 lanes) per ray.
//
// Replaces NeRFRendererDGS.sample_coarse / sample_depthguided / fill_up_uniform_samples
// (reference nerf_renderer.py:39-63, :65-190, :367-397), weighted_mean_n_std (torch_helpers.py:215-223)
// and the three nearest-neighbour lookups SpatialEncoder.index_depth / index_depth_std / index_normal
// (image_encoder.py:148-223, torch_helpers.py:99-159).
//
// Per ray: 1000 (<=1024) stratified candidates, each projected into the NV source views (3 nearest taps
// per view from the small depth / std / normal maps, which stay L2 resident), erf surface likelihood,
// max over views; then inside the wave: exclusive transmittance product (lane-local product + wave
// scan), top-(K-G) selection by a 31-step radix select on the likelihood bits + ballot-free
// compaction, likelihood-weighted mean/std of the candidate depths, G gaussian samples, bitonic sort,
// stratified fill of the empty slots and the final sort.  All candidate state lives in LDS / registers;
// HBM sees 32 B in and 4K B out per ray (plus the optional explicit noise).
#include "common.hpp"

namespace diner {

constexpr int kMaxCand = 1024;
constexpr int kCandPerLane = kMaxCand / kWave;   // 16
constexpr int kMaxK = 256;
constexpr int kRaysPerBlock = 4;

struct SamplerArgs {
  const float* rays;
  const float* t_base;
  const float* noise_coarse;
  const float* noise_gauss;
  const float* noise_fill;
  float* z_out;
  float* z_unfilled;
  uint64_t seed;
  uint32_t ray_key0;       // index of rays[0] in the caller's ray list: the in-kernel noise of ray i is keyed by ray_key0 + i
  int NR, n_cand, K, G;
  float depth_diff_max;
};

// what the info kernels write beside z_out, each only where its pointer is set: the unfilled samples in the reference's slot order
// (picks by descending likelihood, then the gaussian samples), the likelihood and candidate index of every pick slot, and per ray
// (sum L, sum O, mean, sigma) of the gaussian fit
struct SamplerInfo {
  float* z_ordered;   // (NR, K)
  float* slot_L;      // (NR, K - G)
  int* slot_idx;      // (NR, K - G)
  float* stats;       // (NR, 4)
};

// surface likelihood of one candidate in one source view (nerf_renderer.py:107-128)
// kDirHere: the ray direction in this camera is rotated here, where the normal test needs it (dcam unused; dx, dy, dz the world
// direction) -- the wide scene's instances, which keep no per-view array
template <class Scene, bool kDirHere = false>
__device__ __forceinline__ float view_likelihood(const Scene& sc, int v, float px, float py, float pz,
                                                 const float* dcam, float step_size, float ddmax, float dx = 0.0f, float dy = 0.0f,
                                                 float dz = 0.0f) {
  float xc, yc, zc;
  world_to_cam(sc.R[v], sc.t[v], px, py, pz, xc, yc, zc);
  const float u = project_axis(xc, zc, sc.focal[v][0], sc.c[v][0], sc.img_w);
  const float w = project_axis(yc, zc, sc.focal[v][1], sc.c[v][1], sc.img_h);
  const int Ws = sc.Ws, Hs = sc.Hs;
  const size_t plane = (size_t)Hs * Ws;
  // --- depth_std: nearest on the 100px exponentially padded map, zeros outside (image_encoder.py:185-194)
  const float su = __fmul_rn(u, __fdiv_rn((float)Ws, (float)Ws + 2.0f * kStdPad));
  const float sv = __fmul_rn(w, __fdiv_rn((float)Hs, (float)Hs + 2.0f * kStdPad));
  const int jx = nearest_zeros(su, Ws + 2 * kStdPad);
  const int jy = nearest_zeros(sv, Hs + 2 * kStdPad);
  if (jx < 0 || jy < 0) return 0.0f;                 // std == 0 -> masked (nerf_renderer.py:123)
  const int kx = jx < kStdPad ? kStdPad - jx : (jx > Ws + kStdPad - 1 ? jx - (Ws + kStdPad - 1) : 0);
  const int ky = jy < kStdPad ? kStdPad - jy : (jy > Hs + kStdPad - 1 ? jy - (Hs + kStdPad - 1) : 0);
  const int sx = min(max(jx - kStdPad, 0), Ws - 1);
  const int sy = min(max(jy - kStdPad, 0), Hs - 1);
  const int e = max(max(kx, ky) - 1, 0);
  float sd = sc.depth_std[v * plane + (size_t)sy * Ws + sx];
  if (e > 0) sd = __fmul_rn(sd, sc.std_pad_scale[e]);
  if (sd == 0.0f) return 0.0f;
  // --- depth: nearest / border (image_encoder.py:157-167)
  const int ix = nearest_border(u, Ws), iy = nearest_border(w, Hs);
  const float d = sc.depth[v * plane + (size_t)iy * Ws + ix];
  if (!(fabsf(__fsub_rn(d, zc)) < ddmax)) return 0.0f;                       // :122
  // --- normal: nearest / zeros (image_encoder.py:210-220); dot with the ray direction in this camera
  const int nx = nearest_zeros(u, Ws), ny = nearest_zeros(w, Hs);
  if (nx >= 0 && ny >= 0) {
    const float* np_ = sc.normals + (size_t)v * 3 * plane + (size_t)ny * Ws + nx;
    float dhere[3];
    if constexpr (kDirHere) {                                                // :102-103
      dhere[0] = rot_row(sc.R[v] + 0, dx, dy, dz);
      dhere[1] = rot_row(sc.R[v] + 3, dx, dy, dz);
      dhere[2] = rot_row(sc.R[v] + 6, dx, dy, dz);
      dcam = dhere;
    }
    const float cosd = __fadd_rn(__fadd_rn(__fmul_rn(dcam[0], np_[0]), __fmul_rn(dcam[1], np_[plane])),
                                 __fmul_rn(dcam[2], np_[2 * plane]));        // :119
    if (!(cosd <= 0.0f)) return 0.0f;                                        // :121
  }
  const float den = __fmul_rn(sd, 1.41421356237309515f);                     // sigma * np.sqrt(2)
  const float half = __fdiv_rn(step_size, 2.0f);
  const float a = __fdiv_rn(__fsub_rn(__fadd_rn(zc, half), d), den);
  const float b = __fdiv_rn(__fsub_rn(__fsub_rn(zc, half), d), den);
  const float L = fabsf(__fmul_rn(0.5f, __fsub_rn(erff(a), erff(b))));       // :125-128
  return (L == L) ? L : 0.0f;
}

// ---- the wide kernels: one workgroup of kWideThreads per ray (n_cand <= 4096, K <= 1024) --------------
constexpr int kWideThreads = 256;
constexpr int kWideWaves = kWideThreads / kWave;             // 4
constexpr int kWideMaxCand = kWideThreads * kCandPerLane;    // 4096: candidate i at thread i / 16, slot i % 16
constexpr int kLongMaxK = 1024;

// per-wave partials of the workgroup reductions, double-buffered: a reduction writes buffer `par`, waits at one barrier
// and reads it; the next one uses the other buffer, so the reads of this one are done before the buffer is written again
struct WgRed {
  float f[2][kWideWaves];
  int i[2][kWideWaves];
};

__device__ __forceinline__ float wg_sum(float v, float (*buf)[kWideWaves], int& par, int tid) {
  v = wave_sum(v);
  if ((tid & (kWave - 1)) == 0) buf[par][tid >> 6] = v;
  __syncthreads();
  const float s = ((buf[par][0] + buf[par][1]) + buf[par][2]) + buf[par][3];
  par ^= 1;
  return s;
}
__device__ __forceinline__ int wg_sum_i(int v, int (*buf)[kWideWaves], int& par, int tid) {
  v = wave_sum_i(v);
  if ((tid & (kWave - 1)) == 0) buf[par][tid >> 6] = v;
  __syncthreads();
  const int s = buf[par][0] + buf[par][1] + buf[par][2] + buf[par][3];
  par ^= 1;
  return s;
}

// in-LDS bitonic sort (ascending) of n2 (power of two) floats by kThreads threads (one wave: n2 <= 256, one
// workgroup of the wide kernels: n2 <= 1024); every thread of the block calls it (block-uniform control flow)
template <int kThreads = kWave>
__device__ __forceinline__ void bitonic_sort(float* s, int n2, int lane) {
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < n2 / 2; t += kThreads) {
        const int lo = ((t / j) * 2 * j) + (t % j);
        const int hi = lo + j;
        const bool up = ((lo & k) == 0);
        const float a = s[lo], b = s[hi];
        if ((a > b) == up) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  }
}

// in-LDS key/value bitonic sort of n2 (power of two, 1 allowed) pairs: key descending, equal keys by ascending value -- the picks of a
// ray by descending likelihood bits, ties by candidate index as at the cut-off.  Empty pairs (key 0, value -1) compare equal to each
// other and below every pick (picks have key > 0).  Same calling rule as bitonic_sort.
template <int kThreads = kWave>
__device__ __forceinline__ void bitonic_sort_pairs(uint32_t* key, int* val, int n2, int lane) {
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < n2 / 2; t += kThreads) {
        const int lo = ((t / j) * 2 * j) + (t % j);
        const int hi = lo + j;
        const bool fwd = ((lo & k) == 0);
        const uint32_t ka = key[lo], kb = key[hi];
        const int va = val[lo], vb = val[hi];
        const bool a_first = ka > kb || (ka == kb && va < vb);
        const bool b_first = kb > ka || (ka == kb && vb < va);
        if (fwd ? b_first : a_first) { key[lo] = kb; key[hi] = ka; val[lo] = vb; val[hi] = va; }
      }
      __syncthreads();
    }
  }
}

// the info kernels' ordered picks: the want pairs the compaction left in (key, val) sorted, then per slot the candidate's depth from the
// intact Z row into S (empty slot: z = 0, likelihood 0, index -1) and the two per-slot outputs
template <int kThreads>
__device__ __forceinline__ void order_picks(uint32_t* key, int* val, const float* Z, float* S, int want, int w2, int lane, bool live,
                                            const SamplerInfo& info, size_t ray) {
  __syncthreads();
  bitonic_sort_pairs<kThreads>(key, val, w2, lane);
  for (int j = lane; j < want; j += kThreads) {
    const int idx = val[j];
    S[j] = idx >= 0 ? Z[idx] : 0.0f;
    if (live) {
      if (info.slot_L) info.slot_L[ray * want + j] = __uint_as_float(key[j]);
      if (info.slot_idx) info.slot_idx[ray * want + j] = idx;
    }
  }
}

// fill_up_uniform_samples on a K-slot LDS row (nerf_renderer.py:367-397); row padded with +inf to n2.
// kThreads == kWave: one wave per row; kThreads == kWideThreads: one workgroup per row, `red` holds the count's partials.
template <int kThreads = kWave>
__device__ __forceinline__ void fill_and_sort(float* s, int K, int n2, float near, float far, const float* noise_row,
                                              uint64_t seed, int ray, int lane, WgRed* red = nullptr, int par = 0) {
  bitonic_sort<kThreads>(s, n2, lane);                                       // :377
  int m = 0;
  for (int j = lane; j < K; j += kThreads) m += (s[j] == 0.0f);
  if constexpr (kThreads == kWave) m = wave_sum_i(m);                        // :382
  else m = wg_sum_i(m, red->i, par, lane);
  if (m > 0) {
    const float step = __fdiv_rn(__fsub_rn(far, near), (float)m);             // :388
    for (int j = lane; j < K; j += kThreads) {
      if (s[j] == 0.0f) {
        const float u = noise_row ? noise_row[j] : rng_uniform(seed, 2u, (uint32_t)ray, (uint32_t)j);      // (`ray` here: the noise key of the ray)
        float z = __fadd_rn(near, __fmul_rn((float)j, step));                 // :389
        z = __fadd_rn(z, __fmul_rn(u, step));                                 // :390
        s[j] = z;
      }
    }
  }
  __syncthreads();
  bitonic_sort<kThreads>(s, n2, lane);                                       // :396
}

// Scene: SceneDev (1..4 views, the instance every 4-view call runs) or SceneDevWide (5..16 views).  The body is a device function of its
// own: written inside the kernel, the 16-view instance's register allocation left a 64-byte stack slot behind (no scratch access)
// kInfo: the info kernel -- the picks ordered (order_picks, the pairs in the dead L row: keys at [0, 256), indices at [256, 512)) and
// SamplerInfo's outputs written; z_out is the plain kernel's bit for bit (the fill sorts the same multiset)
template <class Scene, bool kInfo = false>
__device__ __forceinline__ void sample_depthguided_body(const Scene& sc, const SamplerArgs& a, const SamplerInfo& info = SamplerInfo{}) {
  __shared__ float sL[kRaysPerBlock][kMaxCand];
  __shared__ float sZ[kRaysPerBlock][kMaxCand];
  __shared__ float sS[kRaysPerBlock][kMaxK];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray_raw = blockIdx.x * kRaysPerBlock + wave;
  const bool live = ray_raw < a.NR;
  const int ray = live ? ray_raw : a.NR - 1;       // dead waves shadow the last ray, control flow stays uniform
  float* L = sL[wave];
  float* Z = sZ[wave];
  float* S = sS[wave];

  const float* r = a.rays + (size_t)ray * 8;
  const float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5], near = r[6], far = r[7];
  const int n_cand = a.n_cand;
  const float step_size = __fdiv_rn(__fsub_rn(far, near), (float)n_cand);       // nerf_renderer.py:95
  const float jitter = (float)(1.0 / (double)n_cand);                           // :53, applied in fp32 at :57

  // the ray direction in each camera (:102-103): four views unrolled into registers once per ray; the wide scene's instance rotates it
  // inside view_likelihood (a dynamically indexed array of 16 views would live in scratch) -- the same rot_row arithmetic either way
  constexpr bool kFew = Scene::kMax <= kMaxViews;
  float dcam[kFew ? kMaxViews : 1][3];
  if constexpr (kFew) {
#pragma unroll
    for (int v = 0; v < kMaxViews; ++v) {                                       // :102-103
      dcam[v][0] = rot_row(sc.R[v] + 0, dx, dy, dz);
      dcam[v][1] = rot_row(sc.R[v] + 3, dx, dy, dz);
      dcam[v][2] = rot_row(sc.R[v] + 6, dx, dy, dz);
    }
  }

  // ---- candidates: lane owns i = lane + 64 c (coalesced noise reads) -----------------------------
  for (int cidx = 0; cidx < kCandPerLane; ++cidx) {
    const int i = lane + kWave * cidx;
    float lk = 0.0f, z = 0.0f;
    if (i < n_cand) {
      const float un = a.noise_coarse ? a.noise_coarse[(size_t)ray * n_cand + i]
                                      : rng_uniform(a.seed, 0u, a.ray_key0 + (uint32_t)ray, (uint32_t)i);
      const float t = __fadd_rn(a.t_base[i], __fmul_rn(un, jitter));            // :57
      z = __fadd_rn(__fmul_rn(near, __fsub_rn(1.0f, t)), __fmul_rn(far, t));    // :60
      const float px = __fadd_rn(ox, __fmul_rn(z, dx));                         // :96
      const float py = __fadd_rn(oy, __fmul_rn(z, dy));
      const float pz = __fadd_rn(oz, __fmul_rn(z, dz));
      for (int v = 0; v < sc.nv; ++v) {
        if constexpr (kFew) {
          lk = fmaxf(lk, view_likelihood(sc, v, px, py, pz, dcam[v], step_size, a.depth_diff_max));   // :129
        } else {
          lk = fmaxf(lk, view_likelihood<Scene, true>(sc, v, px, py, pz, nullptr, step_size, a.depth_diff_max, dx, dy, dz));
        }
      }
    }
    L[i] = lk;
    Z[i] = z;
  }
  __syncthreads();

  // ---- lane-contiguous view: i = 16 lane + k ------------------------------------------------------
  float lv[kCandPerLane], zv[kCandPerLane];
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) {
    lv[k] = L[lane * kCandPerLane + k];
    zv[k] = Z[lane * kCandPerLane + k];
  }
  // exclusive transmittance product  O_i = L_i * prod_{j<i} (1 - L_j)            (:131-132)
  float run = 1.0f;
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) run *= (1.0f - lv[k]);
  float incl = run;                          // inclusive wave scan of the per-lane products
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const float up = __shfl_up(incl, o, kWave);
    if (lane >= o) incl *= up;
  }
  float carry = __shfl_up(incl, 1, kWave);
  if (lane == 0) carry = 1.0f;
  float ov[kCandPerLane];
  float osum = 0.0f;
  int any_o = 0;
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) {
    ov[k] = lv[k] * carry;
    carry *= (1.0f - lv[k]);
    osum += ov[k];
    any_o |= (ov[k] != 0.0f);
  }
  osum = wave_sum(osum);
  const bool has_surface = wave_sum_i(any_o) > 0;                                // :182
  // weighted mean / std of the candidate depths (torch_helpers.py:215-223)
  float mean = 0.0f, sd = 0.0f;
  if (has_surface) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) acc += zv[k] * (ov[k] / osum);
    mean = wave_sum(acc);
    acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) {
      const float dlt = zv[k] - mean;
      acc += (dlt * dlt) * (ov[k] / osum);
    }
    sd = sqrtf(wave_sum(acc));
  }
  if constexpr (kInfo) {
    float lsum = 0.0f;
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) lsum += lv[k];
    lsum = wave_sum(lsum);
    if (info.stats && live && lane == 0) {
      float* st = info.stats + (size_t)ray * 4;
      st[0] = lsum;
      st[1] = osum;
      st[2] = mean;
      st[3] = sd;
    }
  }

  // ---- top-(K-G) by likelihood: radix select on the (non-negative) float bit patterns (:172-178) ----
  const int K = a.K, G = a.G, want = K - G;
  uint32_t ub[kCandPerLane];
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) ub[k] = __float_as_uint(lv[k]);
  uint32_t T = 0;
  if (want > 0) {
    for (int bit = 30; bit >= 0; --bit) {
      const uint32_t trial = T | (1u << bit);
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < kCandPerLane; ++k) cnt += (ub[k] >= trial);
      if (wave_sum_i(cnt) >= want) T = trial;
    }
  }
  // candidates strictly above T are all taken; ties at T (only if T > 0) fill the remainder in index order
  int n_gt = 0, n_eq = 0;
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) {
    n_gt += (ub[k] > T);
    n_eq += (ub[k] == T);
  }
  int pre_gt = n_gt, pre_eq = n_eq;          // inclusive scans over lanes
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int g1 = __shfl_up(pre_gt, o, kWave), e1 = __shfl_up(pre_eq, o, kWave);
    if (lane >= o) { pre_gt += g1; pre_eq += e1; }
  }
  const int tot_gt = __shfl(pre_gt, kWave - 1, kWave);
  const int eq_take = (T > 0 && want > 0) ? max(want - tot_gt, 0) : 0;
  int off_gt = pre_gt - n_gt;
  int off_eq = pre_eq - n_eq;
  for (int j = lane; j < kMaxK; j += kWave) S[j] = (j < K) ? 0.0f : __builtin_inff();
  uint32_t* pkey = reinterpret_cast<uint32_t*>(L);       // kInfo: the L row is dead (lv holds it), Z stays for the depths
  int* pval = reinterpret_cast<int*>(L) + kMaxK;
  int w2 = 1;
  if constexpr (kInfo) {
    while (w2 < want) w2 <<= 1;
    if (want > 0)
      for (int j = lane; j < w2; j += kWave) { pkey[j] = 0u; pval[j] = -1; }
  }
  __syncthreads();
  if (want > 0) {
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) {
      if (ub[k] > T) {
        if constexpr (kInfo) { pkey[off_gt] = ub[k]; pval[off_gt] = lane * kCandPerLane + k; ++off_gt; }
        else S[off_gt++] = zv[k];
      } else if (ub[k] == T && T > 0) {
        if (off_eq < eq_take) {
          if constexpr (kInfo) { pkey[tot_gt + off_eq] = ub[k]; pval[tot_gt + off_eq] = lane * kCandPerLane + k; }
          else S[tot_gt + off_eq] = zv[k];
        }
        ++off_eq;
      }
    }
    if constexpr (kInfo) order_picks<kWave>(pkey, pval, Z, S, want, w2, lane, live, info, (size_t)ray);
  }
  // gaussian samples into the LAST G slots of every ray (zeros when the ray sees no surface)   (:181-190)
  for (int g = lane; g < G; g += kWave) {
    float zg = 0.0f;
    if (has_surface) {
      const float n = a.noise_gauss ? a.noise_gauss[(size_t)ray * G + g]
                                    : rng_normal(a.seed, 1u, a.ray_key0 + (uint32_t)ray, (uint32_t)g);
      zg = __fadd_rn(__fmul_rn(n, sd), mean);                                    // :188
    }
    S[want + g] = zg;
  }
  __syncthreads();
  float* zu = kInfo ? info.z_ordered : a.z_unfilled;
  if (zu && live)
    for (int j = lane; j < K; j += kWave) zu[(size_t)ray * K + j] = S[j];

  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  fill_and_sort(S, K, n2, near, far, a.noise_fill ? a.noise_fill + (size_t)ray * K : nullptr, a.seed, (int)(a.ray_key0 + (uint32_t)ray), lane);
  if (live)
    for (int j = lane; j < K; j += kWave) a.z_out[(size_t)ray * K + j] = S[j];
}

template <class Scene>
__global__ __launch_bounds__(kRaysPerBlock* kWave) void k_sample_depthguided(Scene sc, SamplerArgs a) { sample_depthguided_body(sc, a); }
template <class Scene>
__global__ __launch_bounds__(kRaysPerBlock* kWave) void k_sample_depthguided_info(Scene sc, SamplerArgs a, SamplerInfo info) {
  sample_depthguided_body<Scene, true>(sc, a, info);
}

__global__ __launch_bounds__(kRaysPerBlock* kWave) void k_fill_uniform(const float* z_in, const float* rays, int NR, int K,
                                                                        const float* noise_fill, uint64_t seed,
                                                                        uint32_t ray_key0, float* z_out) {
  __shared__ float sS[kRaysPerBlock][kMaxK];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray_raw = blockIdx.x * kRaysPerBlock + wave;
  const bool live = ray_raw < NR;
  const int ray = live ? ray_raw : NR - 1;
  float* S = sS[wave];
  for (int j = lane; j < kMaxK; j += kWave) S[j] = (j < K) ? z_in[(size_t)ray * K + j] : __builtin_inff();
  __syncthreads();
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  fill_and_sort(S, K, n2, rays[(size_t)ray * 8 + 6], rays[(size_t)ray * 8 + 7],
                noise_fill ? noise_fill + (size_t)ray * K : nullptr, seed, (int)(ray_key0 + (uint32_t)ray), lane);
  if (live)
    for (int j = lane; j < K; j += kWave) z_out[(size_t)ray * K + j] = S[j];
}

// Wide sampler: the per-thread structure of k_sample_depthguided (16 candidates per thread, same arithmetic per candidate)
// with the workgroup as the ray, so n_cand <= 256 x 16 = 4096 and K <= 1024.  The transmittance product, the sums of the
// gaussian fit, the radix-select counts and the compaction offsets are wave scans / sums plus a 4-entry LDS carry.  The
// likelihood bits are view_likelihood's, the pick rule (all candidates above the threshold T, ties at T in index order)
// and the noise keys are the bounded kernel's: a ray's picks and draws do not depend on which kernel ran.
// LDS: 2 x 16 KB candidate rows + 4 KB slot row + the reduction carries (~36 KB, 4 workgroups per CU).
// Info...: empty (the plain kernel, two arguments) or SamplerInfo (the info kernel: as in sample_depthguided_body, the pairs in the
// dead L row, keys at [0, 1024), indices at [1024, 2048)).  The text stays inside the kernel: moved into a device function shared by
// two wrappers, the plain 16-view instance spilt four more SGPRs.
__device__ __forceinline__ SamplerInfo info_of() { return SamplerInfo{}; }
__device__ __forceinline__ SamplerInfo info_of(const SamplerInfo& i) { return i; }
template <class Scene, class... Info>
__global__ __launch_bounds__(kWideThreads) void k_sample_depthguided_wide(Scene sc, SamplerArgs a, Info... extra) {
  constexpr bool kInfo = sizeof...(Info) > 0;
  const SamplerInfo info = info_of(extra...);
  __shared__ float L[kWideMaxCand];
  __shared__ float Z[kWideMaxCand];
  __shared__ float S[kLongMaxK];
  __shared__ WgRed red;
  __shared__ float wprod[kWideWaves];
  __shared__ int wscan[2][kWideWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ray = blockIdx.x;                       // grid == NR: every workgroup has a ray
  int par = 0;

  const float* r = a.rays + (size_t)ray * 8;
  const float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5], near = r[6], far = r[7];
  const int n_cand = a.n_cand;
  const float step_size = __fdiv_rn(__fsub_rn(far, near), (float)n_cand);       // nerf_renderer.py:95
  const float jitter = (float)(1.0 / (double)n_cand);                           // :53, applied in fp32 at :57

  // the ray direction in each camera (:102-103): four views unrolled into registers once per ray; the wide scene's instance rotates it
  // inside view_likelihood (a dynamically indexed array of 16 views would live in scratch) -- the same rot_row arithmetic either way
  constexpr bool kFew = Scene::kMax <= kMaxViews;
  float dcam[kFew ? kMaxViews : 1][3];
  if constexpr (kFew) {
#pragma unroll
    for (int v = 0; v < kMaxViews; ++v) {                                       // :102-103
      dcam[v][0] = rot_row(sc.R[v] + 0, dx, dy, dz);
      dcam[v][1] = rot_row(sc.R[v] + 3, dx, dy, dz);
      dcam[v][2] = rot_row(sc.R[v] + 6, dx, dy, dz);
    }
  }

  // ---- candidates: thread owns i = tid + 256 c (coalesced noise reads); slots >= n_cand are zero -------
  for (int cidx = 0; cidx < kCandPerLane; ++cidx) {
    const int i = tid + kWideThreads * cidx;
    float lk = 0.0f, z = 0.0f;
    if (i < n_cand) {
      const float un = a.noise_coarse ? a.noise_coarse[(size_t)ray * n_cand + i]
                                      : rng_uniform(a.seed, 0u, a.ray_key0 + (uint32_t)ray, (uint32_t)i);
      const float t = __fadd_rn(a.t_base[i], __fmul_rn(un, jitter));            // :57
      z = __fadd_rn(__fmul_rn(near, __fsub_rn(1.0f, t)), __fmul_rn(far, t));    // :60
      const float px = __fadd_rn(ox, __fmul_rn(z, dx));                         // :96
      const float py = __fadd_rn(oy, __fmul_rn(z, dy));
      const float pz = __fadd_rn(oz, __fmul_rn(z, dz));
      for (int v = 0; v < sc.nv; ++v) {
        if constexpr (kFew) {
          lk = fmaxf(lk, view_likelihood(sc, v, px, py, pz, dcam[v], step_size, a.depth_diff_max));   // :129
        } else {
          lk = fmaxf(lk, view_likelihood<Scene, true>(sc, v, px, py, pz, nullptr, step_size, a.depth_diff_max, dx, dy, dz));
        }
      }
    }
    L[i] = lk;
    Z[i] = z;
  }
  for (int j = tid; j < kLongMaxK; j += kWideThreads) S[j] = (j < a.K) ? 0.0f : __builtin_inff();
  __syncthreads();

  // ---- thread-contiguous view: i = 16 tid + k ---------------------------------------------------------
  float lv[kCandPerLane], zv[kCandPerLane];
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) {
    lv[k] = L[tid * kCandPerLane + k];
    zv[k] = Z[tid * kCandPerLane + k];
  }
  // exclusive transmittance product  O_i = L_i * prod_{j<i} (1 - L_j)            (:131-132)
  float run = 1.0f;
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) run *= (1.0f - lv[k]);
  float incl = run;                          // inclusive wave scan of the per-thread products
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const float up = __shfl_up(incl, o, kWave);
    if (lane >= o) incl *= up;
  }
  if (lane == kWave - 1) wprod[wave] = incl;
  float carry = __shfl_up(incl, 1, kWave);
  if (lane == 0) carry = 1.0f;
  __syncthreads();
  float wcarry = 1.0f;                       // product of the earlier waves' totals
  for (int w = 0; w < wave; ++w) wcarry *= wprod[w];
  carry *= wcarry;
  float ov[kCandPerLane];
  float osum = 0.0f;
  int any_o = 0;
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) {
    ov[k] = lv[k] * carry;
    carry *= (1.0f - lv[k]);
    osum += ov[k];
    any_o |= (ov[k] != 0.0f);
  }
  osum = wg_sum(osum, red.f, par, tid);
  const bool has_surface = wg_sum_i(any_o, red.i, par, tid) > 0;                 // :182
  // weighted mean / std of the candidate depths (torch_helpers.py:215-223)
  float mean = 0.0f, sd = 0.0f;
  if (has_surface) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) acc += zv[k] * (ov[k] / osum);
    mean = wg_sum(acc, red.f, par, tid);
    acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) {
      const float dlt = zv[k] - mean;
      acc += (dlt * dlt) * (ov[k] / osum);
    }
    sd = sqrtf(wg_sum(acc, red.f, par, tid));
  }
  if constexpr (kInfo) {
    float lsum = 0.0f;
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) lsum += lv[k];
    lsum = wg_sum(lsum, red.f, par, tid);
    if (info.stats && tid == 0) {
      float* st = info.stats + (size_t)ray * 4;
      st[0] = lsum;
      st[1] = osum;
      st[2] = mean;
      st[3] = sd;
    }
  }

  // ---- top-(K-G) by likelihood: radix select on the (non-negative) float bit patterns (:172-178) ----
  const int K = a.K, G = a.G, want = K - G;
  uint32_t ub[kCandPerLane];
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) ub[k] = __float_as_uint(lv[k]);
  uint32_t T = 0;
  if (want > 0) {
    for (int bit = 30; bit >= 0; --bit) {
      const uint32_t trial = T | (1u << bit);
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < kCandPerLane; ++k) cnt += (ub[k] >= trial);
      if (wg_sum_i(cnt, red.i, par, tid) >= want) T = trial;
    }
  }
  // candidates strictly above T are all taken; ties at T (only if T > 0) fill the remainder in index order
  int n_gt = 0, n_eq = 0;
#pragma unroll
  for (int k = 0; k < kCandPerLane; ++k) {
    n_gt += (ub[k] > T);
    n_eq += (ub[k] == T);
  }
  int pre_gt = n_gt, pre_eq = n_eq;          // inclusive scans over the wave's threads
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int g1 = __shfl_up(pre_gt, o, kWave), e1 = __shfl_up(pre_eq, o, kWave);
    if (lane >= o) { pre_gt += g1; pre_eq += e1; }
  }
  if (lane == kWave - 1) { wscan[0][wave] = pre_gt; wscan[1][wave] = pre_eq; }
  uint32_t* pkey = reinterpret_cast<uint32_t*>(L);       // kInfo: the L row is dead (every thread's lv holds its part), Z stays for the depths
  int* pval = reinterpret_cast<int*>(L) + kLongMaxK;
  int w2 = 1;
  if constexpr (kInfo) {
    while (w2 < want) w2 <<= 1;
    if (want > 0)
      for (int j = tid; j < w2; j += kWideThreads) { pkey[j] = 0u; pval[j] = -1; }
  }
  __syncthreads();
  int base_gt = 0, base_eq = 0, tot_gt = 0;  // earlier waves' totals (exclusive scan over waves) and the ray's total
  for (int w = 0; w < kWideWaves; ++w) {
    if (w < wave) { base_gt += wscan[0][w]; base_eq += wscan[1][w]; }
    tot_gt += wscan[0][w];
  }
  const int eq_take = (T > 0 && want > 0) ? max(want - tot_gt, 0) : 0;
  int off_gt = base_gt + pre_gt - n_gt;
  int off_eq = base_eq + pre_eq - n_eq;
  if (want > 0) {
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) {
      if (ub[k] > T) {
        if constexpr (kInfo) { pkey[off_gt] = ub[k]; pval[off_gt] = tid * kCandPerLane + k; ++off_gt; }
        else S[off_gt++] = zv[k];
      } else if (ub[k] == T && T > 0) {
        if (off_eq < eq_take) {
          if constexpr (kInfo) { pkey[tot_gt + off_eq] = ub[k]; pval[tot_gt + off_eq] = tid * kCandPerLane + k; }
          else S[tot_gt + off_eq] = zv[k];
        }
        ++off_eq;
      }
    }
    if constexpr (kInfo) order_picks<kWideThreads>(pkey, pval, Z, S, want, w2, tid, true, info, (size_t)ray);
  }
  // gaussian samples into the LAST G slots of every ray (zeros when the ray sees no surface)   (:181-190)
  for (int g = tid; g < G; g += kWideThreads) {
    float zg = 0.0f;
    if (has_surface) {
      const float n = a.noise_gauss ? a.noise_gauss[(size_t)ray * G + g]
                                    : rng_normal(a.seed, 1u, a.ray_key0 + (uint32_t)ray, (uint32_t)g);
      zg = __fadd_rn(__fmul_rn(n, sd), mean);                                    // :188
    }
    S[want + g] = zg;
  }
  __syncthreads();
  float* zu = kInfo ? info.z_ordered : a.z_unfilled;
  if (zu)
    for (int j = tid; j < K; j += kWideThreads) zu[(size_t)ray * K + j] = S[j];
  __syncthreads();      // the four waves share S: the sort below must not swap slots another wave has yet to copy out

  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  fill_and_sort<kWideThreads>(S, K, n2, near, far, a.noise_fill ? a.noise_fill + (size_t)ray * K : nullptr, a.seed,
                              (int)(a.ray_key0 + (uint32_t)ray), tid, &red, par);
  for (int j = tid; j < K; j += kWideThreads) a.z_out[(size_t)ray * K + j] = S[j];
}

// fill_up_uniform_samples alone on rows of up to 1024 slots: one workgroup per ray, the wide kernel's sort
__global__ __launch_bounds__(kWideThreads) void k_fill_uniform_wide(const float* z_in, const float* rays, int K,
                                                                   const float* noise_fill, uint64_t seed,
                                                                   uint32_t ray_key0, float* z_out) {
  __shared__ float S[kLongMaxK];
  __shared__ WgRed red;
  const int tid = threadIdx.x, ray = blockIdx.x;
  for (int j = tid; j < kLongMaxK; j += kWideThreads) S[j] = (j < K) ? z_in[(size_t)ray * K + j] : __builtin_inff();
  __syncthreads();
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  fill_and_sort<kWideThreads>(S, K, n2, rays[(size_t)ray * 8 + 6], rays[(size_t)ray * 8 + 7],
                              noise_fill ? noise_fill + (size_t)ray * K : nullptr, seed, (int)(ray_key0 + (uint32_t)ray), tid,
                              &red);
  for (int j = tid; j < K; j += kWideThreads) z_out[(size_t)ray * K + j] = S[j];
}

// the scene's cameras into the kernel arguments and the launch: 1..4 views on the SceneDev instance (the kernels as they were before the
// wide scene existed), 5..16 on the SceneDevWide one
template <class Scene>
static int launch_sampler(const DinerScene* scene, const SamplerArgs& a, bool wide, const char* who, hipStream_t stream,
                          const SamplerInfo* info) {
  Scene sd;
  int rc = make_scene_dev(scene, &sd);
  if (rc) return rc;
  DINER_CHECK_ARG(scene->depth && scene->depth_std && scene->normals && scene->std_pad_scale, "%s: scene depth/std/normal maps missing", who);
  const dim3 grid_b((a.NR + kRaysPerBlock - 1) / kRaysPerBlock), block_b(kRaysPerBlock * kWave);
  if (info && wide)
    hipLaunchKernelGGL((k_sample_depthguided_wide<Scene, SamplerInfo>), dim3(a.NR), dim3(kWideThreads), 0, stream, sd, a, *info);
  else if (info)
    hipLaunchKernelGGL(k_sample_depthguided_info<Scene>, grid_b, block_b, 0, stream, sd, a, *info);
  else if (wide)
    hipLaunchKernelGGL(k_sample_depthguided_wide<Scene>, dim3(a.NR), dim3(kWideThreads), 0, stream, sd, a);
  else
    hipLaunchKernelGGL(k_sample_depthguided<Scene>, dim3((a.NR + kRaysPerBlock - 1) / kRaysPerBlock), dim3(kRaysPerBlock * kWave), 0,
                       stream, sd, a);
  DINER_LAUNCH_OK();
  return 0;
}
static int sample(const DinerScene* scene, const SamplerArgs& a, bool wide, const char* who, hipStream_t stream,
                  const SamplerInfo* info = nullptr) {
  DINER_CHECK_ARG(scene->nv >= 1 && scene->nv <= kMaxViewsWide, "scene: nv=%d outside [1,%d]", scene->nv, kMaxViewsWide);
  return scene->nv <= kMaxViews ? launch_sampler<SceneDev>(scene, a, wide, who, stream, info)
                                : launch_sampler<SceneDevWide>(scene, a, wide, who, stream, info);
}

// the checks of diner_sample_depthguided_f32 / _long_f32 (max_cand, max_k: the entry's limits) for the info entries, then the launch
static int sample_info(const char* who, int max_cand, int max_k, const DinerScene* scene, const float* rays, int NR, int n_cand, int K,
                       int G, float depth_diff_max, const float* t_base, const float* noise_coarse, const float* noise_gauss,
                       const float* noise_fill, uint64_t seed, long long ray_index0, float* z_out, const SamplerInfo& info,
                       void* stream) {
  DINER_CHECK_ARG(scene && rays && t_base && z_out, "%s: null pointer argument", who);
  DINER_CHECK_ARG(NR > 0, "%s: NR must be positive (got %d)", who, NR);
  DINER_CHECK_ARG(n_cand > 0 && n_cand <= max_cand, "%s: n_cand=%d outside [1,%d]", who, n_cand, max_cand);
  DINER_CHECK_ARG(K > 0 && K <= max_k, "%s: n_samples K=%d outside [1,%d]", who, K, max_k);
  DINER_CHECK_ARG(G >= 0 && G <= K, "%s: need 0 <= n_gaussian <= n_samples (got G=%d, K=%d)", who, G, K);
  DINER_CHECK_ARG(ray_index0 >= 0 && ray_index0 + NR <= (1ll << 32),
                  "%s: ray_index0 = %lld outside [0, 2^32 - NR] (the noise key of a ray is a 32-bit index)", who, ray_index0);
  SamplerArgs a{rays, t_base, noise_coarse, noise_gauss, noise_fill, z_out, nullptr, seed, (uint32_t)ray_index0, NR, n_cand, K,
                G, depth_diff_max};
  return sample(scene, a, !(K <= kMaxK && n_cand <= kMaxCand), who, (hipStream_t)stream, &info);
}
}  // namespace diner

using namespace diner;

extern "C" int diner_sample_depthguided_f32(const DinerScene* scene, const float* rays, int NR, int n_cand, int K,
                                            int G, float depth_diff_max, const float* t_base,
                                            const float* noise_coarse, const float* noise_gauss,
                                            const float* noise_fill, uint64_t seed, long long ray_index0, float* z_out,
                                            float* z_unfilled, void* stream) {
  DINER_CHECK_ARG(scene && rays && t_base && z_out, "sample_depthguided: null pointer argument");
  DINER_CHECK_ARG(NR > 0, "sample_depthguided: NR must be positive (got %d)", NR);
  DINER_CHECK_ARG(n_cand > 0 && n_cand <= kMaxCand, "sample_depthguided: n_cand=%d outside [1,%d]", n_cand, kMaxCand);
  DINER_CHECK_ARG(K > 0 && K <= kMaxK, "sample_depthguided: n_samples=%d outside [1,%d]", K, kMaxK);
  DINER_CHECK_ARG(G >= 0 && G <= K, "sample_depthguided: need 0 <= n_gaussian <= n_samples (got %d, %d)", G, K);
  DINER_CHECK_ARG(ray_index0 >= 0 && ray_index0 + NR <= (1ll << 32),
                  "sample_depthguided: ray_index0 = %lld outside [0, 2^32 - NR] (the noise key of a ray is a 32-bit index)", ray_index0);
  SamplerArgs a{rays, t_base, noise_coarse, noise_gauss, noise_fill, z_out, z_unfilled, seed, (uint32_t)ray_index0, NR, n_cand, K,
                G, depth_diff_max};
  return sample(scene, a, false, "sample_depthguided", (hipStream_t)stream);
}

extern "C" int diner_fill_uniform_f32(const float* z_in, const float* rays, int NR, int K, const float* noise_fill,
                                      uint64_t seed, long long ray_index0, float* z_out, void* stream) {
  DINER_CHECK_ARG(z_in && rays && z_out, "fill_uniform: null pointer argument");
  DINER_CHECK_ARG(NR > 0 && K > 0 && K <= kMaxK, "fill_uniform: bad sizes NR=%d K=%d", NR, K);
  DINER_CHECK_ARG(ray_index0 >= 0 && ray_index0 + NR <= (1ll << 32),
                  "fill_uniform: ray_index0 = %lld outside [0, 2^32 - NR] (the noise key of a ray is a 32-bit index)", ray_index0);
  const int blocks = (NR + kRaysPerBlock - 1) / kRaysPerBlock;
  hipLaunchKernelGGL(k_fill_uniform, dim3(blocks), dim3(kRaysPerBlock * kWave), 0, (hipStream_t)stream, z_in, rays, NR,
                     K, noise_fill, seed, (uint32_t)ray_index0, z_out);
  DINER_LAUNCH_OK();
  return 0;
}

// ---- long entries: the whole range, the kernel picked from the sizes.  Where the bounded kernels fit (K <= 256,
// n_cand <= 1024) they run with the same arguments, so results there are bit-identical to the bounded entries.
extern "C" int diner_sample_depthguided_long_f32(const DinerScene* scene, const float* rays, int NR, int n_cand, int K,
                                                 int G, float depth_diff_max, const float* t_base,
                                                 const float* noise_coarse, const float* noise_gauss,
                                                 const float* noise_fill, uint64_t seed, long long ray_index0,
                                                 float* z_out, float* z_unfilled, void* stream) {
  DINER_CHECK_ARG(scene && rays && t_base && z_out, "sample_depthguided_long: null pointer argument");
  DINER_CHECK_ARG(NR > 0, "sample_depthguided_long: NR must be positive (got %d)", NR);
  DINER_CHECK_ARG(n_cand > 0 && n_cand <= kWideMaxCand, "sample_depthguided_long: n_cand=%d outside [1,%d]", n_cand,
                  kWideMaxCand);
  DINER_CHECK_ARG(K > 0 && K <= kLongMaxK, "sample_depthguided_long: n_samples K=%d outside [1,%d]", K, kLongMaxK);
  DINER_CHECK_ARG(G >= 0 && G <= K, "sample_depthguided_long: need 0 <= n_gaussian <= n_samples (got G=%d, K=%d)", G, K);
  DINER_CHECK_ARG(ray_index0 >= 0 && ray_index0 + NR <= (1ll << 32),
                  "sample_depthguided_long: ray_index0 = %lld outside [0, 2^32 - NR] (the noise key of a ray is a 32-bit index)",
                  ray_index0);
  if (K <= kMaxK && n_cand <= kMaxCand)
    return diner_sample_depthguided_f32(scene, rays, NR, n_cand, K, G, depth_diff_max, t_base, noise_coarse, noise_gauss,
                                        noise_fill, seed, ray_index0, z_out, z_unfilled, stream);
  SamplerArgs a{rays, t_base, noise_coarse, noise_gauss, noise_fill, z_out, z_unfilled, seed, (uint32_t)ray_index0, NR, n_cand, K,
                G, depth_diff_max};
  return sample(scene, a, true, "sample_depthguided_long", (hipStream_t)stream);
}

extern "C" int diner_sample_depthguided_info_f32(const DinerScene* scene, const float* rays, int NR, int n_cand, int K, int G,
                                                 float depth_diff_max, const float* t_base, const float* noise_coarse,
                                                 const float* noise_gauss, const float* noise_fill, uint64_t seed,
                                                 long long ray_index0, float* z_out, float* z_ordered, float* slot_L,
                                                 int32_t* slot_idx, float* stats, void* stream) {
  return sample_info("sample_depthguided_info", kMaxCand, kMaxK, scene, rays, NR, n_cand, K, G, depth_diff_max, t_base, noise_coarse,
                     noise_gauss, noise_fill, seed, ray_index0, z_out, SamplerInfo{z_ordered, slot_L, slot_idx, stats}, stream);
}

// the bounded info kernel where it fits, as the plain long entry picks the bounded kernel
extern "C" int diner_sample_depthguided_info_long_f32(const DinerScene* scene, const float* rays, int NR, int n_cand, int K, int G,
                                                      float depth_diff_max, const float* t_base, const float* noise_coarse,
                                                      const float* noise_gauss, const float* noise_fill, uint64_t seed,
                                                      long long ray_index0, float* z_out, float* z_ordered, float* slot_L,
                                                      int32_t* slot_idx, float* stats, void* stream) {
  return sample_info("sample_depthguided_info_long", kWideMaxCand, kLongMaxK, scene, rays, NR, n_cand, K, G, depth_diff_max, t_base,
                     noise_coarse, noise_gauss, noise_fill, seed, ray_index0, z_out, SamplerInfo{z_ordered, slot_L, slot_idx, stats},
                     stream);
}

extern "C" int diner_fill_uniform_long_f32(const float* z_in, const float* rays, int NR, int K, const float* noise_fill,
                                           uint64_t seed, long long ray_index0, float* z_out, void* stream) {
  DINER_CHECK_ARG(z_in && rays && z_out, "fill_uniform_long: null pointer argument");
  DINER_CHECK_ARG(NR > 0 && K > 0 && K <= kLongMaxK, "fill_uniform_long: bad sizes NR=%d K=%d (K <= %d)", NR, K, kLongMaxK);
  DINER_CHECK_ARG(ray_index0 >= 0 && ray_index0 + NR <= (1ll << 32),
                  "fill_uniform_long: ray_index0 = %lld outside [0, 2^32 - NR] (the noise key of a ray is a 32-bit index)", ray_index0);
  if (K <= kMaxK) return diner_fill_uniform_f32(z_in, rays, NR, K, noise_fill, seed, ray_index0, z_out, stream);
  hipLaunchKernelGGL(k_fill_uniform_wide, dim3(NR), dim3(kWideThreads), 0, (hipStream_t)stream, z_in, rays, K, noise_fill,
                     seed, (uint32_t)ray_index0, z_out);
  DINER_LAUNCH_OK();
  return 0;
}
