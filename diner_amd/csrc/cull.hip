// Empty-ray culling: keep the rays the depth maps put a surface on, and put their results back into the frame.
//
// diner_compact_live_f32: order-preserving stream compaction of one sampler batch, appended to a frame-level list.  A ray is live iff
// !(stats[i][1] <= threshold) -- stats as the info sampler writes it, [1] = sum O, the depth maps' probability that the ray meets a
// surface (the reference's ray_mask, nerf_renderer.py:182, at threshold 0); a NaN is live.  Three launches on the caller's stream, the
// stream being the only ordering between workgroups (none waits on another): live rays per block of kCullThreads rays -> one workgroup
// scans the block counts, reads the frame's counter as the base and advances it -> every block scans its own flags again and copies
// its live rows.  Integer arithmetic only: the bytes written are a function of the inputs alone, and a ray list split into consecutive
// calls gives the bytes of the one call.
//
// diner_expand_live_f32: out[i] = slot[i] < 0 ? bg : tiles[slot[i]], one thread per output value.
#include "common.hpp"

namespace diner {

namespace {

constexpr int kCullThreads = 256;                // rays per workgroup of the count / scatter kernels
constexpr int kCullWaves = kCullThreads / kWave;

__device__ __forceinline__ bool ray_live(const float* __restrict__ stats, int i, float threshold) {
  return !(stats[(size_t)i * 4 + 1] <= threshold);
}

// Inclusive sum over the workgroup in thread order; `red` (kCullWaves ints) is reused by the next call after its trailing barrier.
__device__ __forceinline__ int block_scan_incl(int v, int* red, int* total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int u = __shfl_up(v, o, kWave);
    if (lane >= o) v += u;
  }
  if (lane == kWave - 1) red[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kCullWaves; ++w) {
    const int c = red[w];
    if (w < wave) before += c;
    all += c;
  }
  __syncthreads();
  *total = all;
  return v + before;
}

__global__ void __launch_bounds__(kCullThreads) k_cull_count(const float* __restrict__ stats, float threshold, int NR,
                                                             int* __restrict__ counts) {
  __shared__ int red[kCullWaves];
  const int i = blockIdx.x * kCullThreads + threadIdx.x;
  const int live = (i < NR && ray_live(stats, i, threshold)) ? 1 : 0;
  int total;
  block_scan_incl(live, red, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// One workgroup: counts[b] -> the row block b's first live ray goes to (*n_live + the live rays of the blocks before it), then
// *n_live += the batch's live rays.  The counter is a 32-bit integer updated by one thread of one workgroup per launch.
__global__ void __launch_bounds__(kCullThreads) k_cull_scan(int* __restrict__ counts, int n_blocks, int* __restrict__ n_live) {
  __shared__ int red[kCullWaves];
  int carry = *n_live;
  for (int b0 = 0; b0 < n_blocks; b0 += kCullThreads) {
    const int b = b0 + threadIdx.x;
    const int v = b < n_blocks ? counts[b] : 0;
    int total;
    const int incl = block_scan_incl(v, red, &total);
    if (b < n_blocks) counts[b] = carry + incl - v;
    carry += total;
  }
  __syncthreads();                                // every thread has read *n_live
  if (threadIdx.x == 0) *n_live = carry;
}

// Rows [0, n_rows) of the block's source rays to their slots.  VEC: row_len is a multiple of 4 and both bases are 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ void copy_rows(const float* __restrict__ src, float* __restrict__ dst, int row_len, int ray0, int n_rows,
                                          const int* __restrict__ s_slot) {
  if (VEC) {
    const int q = row_len >> 2;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src) + (size_t)ray0 * q;
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
    const int n = n_rows * q;
    for (int it = threadIdx.x; it < n; it += kCullThreads) {
      const int r = it / q, c = it - r * q;
      const int sl = s_slot[r];
      if (sl >= 0) d4[(size_t)sl * q + c] = s4[it];
    }
  } else {
    const float* __restrict__ s = src + (size_t)ray0 * row_len;
    const long long n = (long long)n_rows * row_len;
    for (long long it = threadIdx.x; it < n; it += kCullThreads) {
      const int r = (int)(it / row_len), c = (int)(it - (long long)r * row_len);
      const int sl = s_slot[r];
      if (sl >= 0) dst[(size_t)sl * row_len + c] = s[it];
    }
  }
}

template <bool VEC_R, bool VEC_Z>
__global__ void __launch_bounds__(kCullThreads) k_cull_scatter(const float* __restrict__ stats, float threshold,
                                                               const float* __restrict__ rays, const float* __restrict__ z, int NR, int K,
                                                               int ray_index0, long long capacity, const int* __restrict__ offsets,
                                                               float* __restrict__ rays_out, float* __restrict__ z_out,
                                                               int* __restrict__ live_idx, int* __restrict__ slot) {
  __shared__ int red[kCullWaves];
  __shared__ int s_slot[kCullThreads];
  const int ray0 = blockIdx.x * kCullThreads;
  const int i = ray0 + threadIdx.x;
  const int live = (i < NR && ray_live(stats, i, threshold)) ? 1 : 0;
  int total;
  const int incl = block_scan_incl(live, red, &total);
  const long long row = (long long)offsets[blockIdx.x] + incl - live;
  const int sl = (live && row >= 0 && row < capacity) ? (int)row : -1;       // a row at or beyond capacity is not written
  s_slot[threadIdx.x] = sl;
  if (i < NR) {
    slot[i] = sl;
    if (sl >= 0) live_idx[sl] = ray_index0 + i;
  }
  __syncthreads();
  if (total == 0) return;                         // uniform across the workgroup
  const int n_rows = min(kCullThreads, NR - ray0);
  copy_rows<VEC_R>(rays, rays_out, 8, ray0, n_rows, s_slot);
  copy_rows<VEC_Z>(z, z_out, K, ray0, n_rows, s_slot);
}

template <int C>
__global__ void __launch_bounds__(256) k_expand_live(const float* __restrict__ tiles, long long n_tiles, const int* __restrict__ slot,
                                                     const float* __restrict__ bg, long long n_values, float* __restrict__ out) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n_values) return;
  const long long i = v / C;
  const int c = (int)(v - i * C);
  const int sl = slot[i];
  out[v] = (sl >= 0 && sl < n_tiles) ? tiles[(size_t)sl * C + c] : bg[c];   // a slot outside the tile list reads nothing
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" size_t diner_compact_live_workspace_bytes(long long NR) {
  if (NR < 1 || NR > 0x7fffffffLL) return 0;
  return (size_t)((NR + kCullThreads - 1) / kCullThreads) * sizeof(int);
}

extern "C" int diner_compact_live_f32(const float* stats, float threshold, const float* rays, const float* z, int NR, int K,
                                      long long ray_index0, long long capacity, float* rays_out, float* z_out, int* live_idx,
                                      int* slot, int* n_live, void* workspace, void* stream) {
  DINER_CHECK_ARG(stats && rays && z && slot && n_live && workspace, "compact_live: null pointer");
  DINER_CHECK_ARG(NR >= 1, "compact_live: NR = %d (need >= 1)", NR);
  DINER_CHECK_ARG(K >= 1 && K <= 1024, "compact_live: K = %d outside [1, 1024]", K);
  DINER_CHECK_ARG(capacity >= 0 && capacity <= 0x7fffffffLL, "compact_live: capacity %lld outside [0, 2^31)", capacity);
  DINER_CHECK_ARG(capacity == 0 || (rays_out && z_out && live_idx), "compact_live: null output with capacity %lld", capacity);
  DINER_CHECK_ARG(ray_index0 >= 0 && ray_index0 + (long long)NR <= 0x7fffffffLL,
                  "compact_live: ray indices [%lld, %lld) do not fit the int32 live_idx", ray_index0, ray_index0 + (long long)NR);
  hipStream_t st = (hipStream_t)stream;
  const int n_blocks = (NR + kCullThreads - 1) / kCullThreads;
  int* counts = static_cast<int*>(workspace);
  hipLaunchKernelGGL(k_cull_count, dim3(n_blocks), dim3(kCullThreads), 0, st, stats, threshold, NR, counts);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(kCullThreads), 0, st, counts, n_blocks, n_live);
  DINER_LAUNCH_OK();
  const bool vr = aligned16(rays) && aligned16(rays_out);
  const bool vz = (K & 3) == 0 && aligned16(z) && aligned16(z_out);
#define DINER_CULL_SCATTER(VR, VZ)                                                                                                  \
  hipLaunchKernelGGL((k_cull_scatter<VR, VZ>), dim3(n_blocks), dim3(kCullThreads), 0, st, stats, threshold, rays, z, NR, K,          \
                     (int)ray_index0, capacity, (const int*)counts, rays_out, z_out, live_idx, slot)
  if (vr && vz) DINER_CULL_SCATTER(true, true);
  else if (vr) DINER_CULL_SCATTER(true, false);
  else if (vz) DINER_CULL_SCATTER(false, true);
  else DINER_CULL_SCATTER(false, false);
#undef DINER_CULL_SCATTER
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_expand_live_f32(const float* tiles, long long n_tiles, const int* slot, const float* bg, long long N, int C,
                                     float* out, void* stream) {
  DINER_CHECK_ARG(slot && bg && out, "expand_live: null pointer");
  DINER_CHECK_ARG(n_tiles >= 0 && n_tiles <= 0x7fffffffLL && (n_tiles == 0 || tiles), "expand_live: %lld tiles without a tile list", n_tiles);
  DINER_CHECK_ARG(N >= 1 && N <= 0x7fffffffLL, "expand_live: N = %lld outside [1, 2^31)", N);
  DINER_CHECK_ARG(C >= 1 && C <= 8, "expand_live: C = %d outside [1, 8]", C);
  hipStream_t st = (hipStream_t)stream;
  const long long n_values = N * C;
  const unsigned grid = (unsigned)((n_values + 255) / 256);
#define DINER_EXPAND(CC)                                                                                                   \
  case CC:                                                                                                                 \
    hipLaunchKernelGGL(k_expand_live<CC>, dim3(grid), dim3(256), 0, st, tiles, n_tiles, slot, bg, n_values, out);         \
    break
  switch (C) {
    DINER_EXPAND(1);
    DINER_EXPAND(2);
    DINER_EXPAND(3);
    DINER_EXPAND(4);
    DINER_EXPAND(5);
    DINER_EXPAND(6);
    DINER_EXPAND(7);
    DINER_EXPAND(8);
  }
#undef DINER_EXPAND
  DINER_LAUNCH_OK();
  return 0;
}
