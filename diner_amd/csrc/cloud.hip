// Nearest neighbour between two clouds of millions of points through a uniform grid, and the sums the distance scores (accuracy,
// completeness, Chamfer, precision / recall / F-score, normal consistency) are made of.
//
// The grid is a counting sort of the target's indices by cell: k_cloud_count (32-bit integer atomics), an exclusive scan in three
// launches (per-block sums, k_cloud_scan_blocks -- the shape of surface.hip's k_surf_scan --, per-block offsets), k_cloud_scatter through
// per-cell cursors.  The scatter also leaves every point next to its index (16 bytes), so a query reads a run of cells as one run of
// memory.  Which of a cell's points comes first is up to the atomics; a query compares (d2, index) pairs, so no output shows it.
//
// k_cloud_nearest: one thread per query.  It visits the cells of Chebyshev ring r around its own (unclamped) cell, r = r0, r0 + 1, ...,
// and after each ring asks whether an unvisited cell can still hold a winner.  An unvisited cell lies beyond one of the (up to six)
// faces of the visited cube that have cells behind them, so the smallest distance to such a face bounds every unvisited point from
// below -- if the face is where the BINNING put it.  floor(fl(fl(p - lo) / h)) >= k holds for p - lo >= k h (1 - 3 u), not k h (u = 2^-24),
// and the fp32 d2 of a point at distance D is above D^2 (1 - 6 u): the bound is computed in double from faces moved by 4e-7 relative
// towards the query and is compared after a further 1e-6 relative and an absolute 4e-38 (below that fp32 products lose their relative
// accuracy).  Clamping only ever widens the outermost cells outwards, and those have no face on that side.
#include "common.hpp"

#include <cmath>
#include <limits>

namespace diner {

namespace {

constexpr int kCloudThreads = 256;
constexpr int kCloudWaves = kCloudThreads / kWave;
constexpr int kScanItems = 4;                                   // consecutive cells a thread of the scan owns
constexpr int kScanTile = kCloudThreads * kScanItems;           // cells a workgroup of the scan owns
constexpr int kReduceBlocks = 1024;                             // most workgroups of k_cloud_reduce
constexpr int kReduceSlot = DINER_CLOUD_REDUCE_OUT;
constexpr long long kCloudMaxPoints = 0x7fffffffLL;
constexpr float kCellFar = 536870912.0f;                        // 2^29: a query's cell coordinate is kept within +- this

// ---- the workspace of a grid: offsets in bytes --------------------------------------------------------------------------------------
struct CloudLayout {
  long long cells, n_tiles;
  size_t cursor, start, tile_sums, order, points, bytes;        // cursor (cells + 1), start (cells + 2), tile_sums (n_tiles) int32;
};                                                              // order (NB) int32; points (NB) int4 {x, y, z bits, index}

bool cloud_dims_ok(int Gx, int Gy, int Gz) {
  return Gx >= 1 && Gy >= 1 && Gz >= 1 && Gx <= DINER_CLOUD_MAX_DIM && Gy <= DINER_CLOUD_MAX_DIM && Gz <= DINER_CLOUD_MAX_DIM &&
         (long long)Gx * Gy * Gz <= (long long)DINER_CLOUD_MAX_CELLS;
}
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
bool cloud_layout(long long NB, int Gx, int Gy, int Gz, CloudLayout* L) {
  if (NB < 1 || NB > kCloudMaxPoints || !cloud_dims_ok(Gx, Gy, Gz)) return false;
  L->cells = (long long)Gx * Gy * Gz;
  L->n_tiles = (L->cells + 1 + kScanTile - 1) / kScanTile;      // the scan runs over cells + 1 counts: the last is the non-finite points'
  L->cursor = 0;
  L->start = align16(L->cursor + (size_t)(L->cells + 1) * 4);
  L->tile_sums = align16(L->start + (size_t)(L->cells + 2) * 4);
  L->order = align16(L->tile_sums + (size_t)L->n_tiles * 4);
  L->points = align16(L->order + (size_t)NB * 4);
  L->bytes = L->points + (size_t)NB * 16;
  return true;
}

struct CloudBox {
  float lo0, lo1, lo2, h;
  int G0, G1, G2;
};

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) <= 3.4028234664e38f && fabsf(y) <= 3.4028234664e38f && fabsf(z) <= 3.4028234664e38f;      // false for a NaN
}
__device__ __forceinline__ int cell_axis(float p, float lo, float h, int G) {
  const float t = floorf(__fdiv_rn(__fsub_rn(p, lo), h));
  return (int)fminf(fmaxf(t, 0.0f), (float)(G - 1));
}
// the cell of a target point; `cells` (behind the last one) for a point with a non-finite coordinate
__device__ __forceinline__ int cell_of(const CloudBox& b, int cells, float x, float y, float z) {
  if (!finite3(x, y, z)) return cells;
  return (cell_axis(z, b.lo2, b.h, b.G2) * b.G1 + cell_axis(y, b.lo1, b.h, b.G1)) * b.G0 + cell_axis(x, b.lo0, b.h, b.G0);
}

__global__ void __launch_bounds__(kCloudThreads) k_cloud_count(const float* __restrict__ xyz, int NB, CloudBox box, int cells,
                                                               int* __restrict__ counts) {
  const long long i = blockIdx.x * (long long)kCloudThreads + threadIdx.x;
  if (i >= NB) return;
  atomicAdd(&counts[cell_of(box, cells, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])], 1);
}

// Inclusive scan over the workgroup (surface.hip's surf_scan_incl); *total = the sum over all of it.
__device__ __forceinline__ int cloud_scan_incl(int v, int* red, int* total) {
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
  for (int w = 0; w < kCloudWaves; ++w) {
    const int c = red[w];
    if (w < wave) before += c;
    all += c;
  }
  __syncthreads();
  *total = all;
  return v + before;
}

// tile_sums[b] = the number of points in the kScanTile cells of workgroup b
__global__ void __launch_bounds__(kCloudThreads) k_cloud_tile_sums(const int* __restrict__ counts, long long n, int* __restrict__ tile_sums) {
  __shared__ int red[kCloudWaves];
  const long long i0 = ((long long)blockIdx.x * kCloudThreads + threadIdx.x) * kScanItems;
  int s = 0;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) s += i0 + q < n ? counts[i0 + q] : 0;
  int total;
  cloud_scan_incl(s, red, &total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// One workgroup: tile_sums[b] -> the number of points before tile b, kCloudThreads tiles a pass.
__global__ void __launch_bounds__(kCloudThreads) k_cloud_scan_blocks(int* __restrict__ tile_sums, long long n_tiles) {
  __shared__ int red[kCloudWaves];
  int carry = 0;
  for (long long b0 = 0; b0 < n_tiles; b0 += kCloudThreads) {
    const long long b = b0 + threadIdx.x;
    const int c = b < n_tiles ? tile_sums[b] : 0;
    int total;
    const int incl = cloud_scan_incl(c, red, &total);
    if (b < n_tiles) tile_sums[b] = carry + incl - c;
    carry += total;
  }
}

// start[i] = cursor[i] = the number of points in cells before i, i < n; start[n] = all of them (counts aliases cursor: each thread reads
// its own cells before it writes them)
__global__ void __launch_bounds__(kCloudThreads) k_cloud_scan_cells(int* __restrict__ cursor, long long n, const int* __restrict__ tile_sums,
                                                                    int* __restrict__ start) {
  __shared__ int red[kCloudWaves];
  const long long i0 = ((long long)blockIdx.x * kCloudThreads + threadIdx.x) * kScanItems;
  int c[kScanItems], s = 0;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    c[q] = i0 + q < n ? cursor[i0 + q] : 0;
    s += c[q];
  }
  int total;
  int at = tile_sums[blockIdx.x] + cloud_scan_incl(s, red, &total) - s;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    if (i0 + q < n) {
      start[i0 + q] = at;
      cursor[i0 + q] = at;
      at += c[q];
      if (i0 + q == n - 1) start[n] = at;
    }
  }
}

__global__ void __launch_bounds__(kCloudThreads) k_cloud_scatter(const float* __restrict__ xyz, int NB, CloudBox box, int cells,
                                                                 int* __restrict__ cursor, int* __restrict__ order, int4* __restrict__ points) {
  const long long i = blockIdx.x * (long long)kCloudThreads + threadIdx.x;
  if (i >= NB) return;
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  const int at = atomicAdd(&cursor[cell_of(box, cells, x, y, z)], 1);
  if (at < 0 || at >= NB) return;                              // cannot happen on the counts of the same cloud: never write outside
  order[at] = (int)i;
  points[at] = make_int4(__float_as_int(x), __float_as_int(y), __float_as_int(z), (int)i);
}

struct CloudBest {
  float d2;
  int idx;
};
// the points at [s, e) of the sorted array against the query
__device__ __forceinline__ void scan_run(const int4* __restrict__ points, int s, int e, float ax, float ay, float az, float cap2,
                                         CloudBest& best) {
  for (int p = s; p < e; ++p) {
    const int4 b = points[p];
    const float dx = __fsub_rn(__int_as_float(b.x), ax), dy = __fsub_rn(__int_as_float(b.y), ay), dz = __fsub_rn(__int_as_float(b.z), az);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    if (d2 <= cap2 && (d2 < best.d2 || (d2 == best.d2 && b.w < best.idx))) {
      best.d2 = d2;
      best.idx = b.w;
    }
  }
}

__global__ void __launch_bounds__(kCloudThreads) k_cloud_nearest(const int* __restrict__ start, const int4* __restrict__ points, CloudBox box,
                                                                 const float* __restrict__ xyz_a, int NA, const int* __restrict__ order,
                                                                 float cap2, float* __restrict__ d2_out, int* __restrict__ idx_out) {
  const long long t = blockIdx.x * (long long)kCloudThreads + threadIdx.x;
  if (t >= NA) return;
  long long q = t;
  if (order) {
    q = order[t];
    if (q < 0 || q >= NA) return;
  }
  const float a[3] = {xyz_a[3 * q], xyz_a[3 * q + 1], xyz_a[3 * q + 2]};
  const float inf = std::numeric_limits<float>::infinity();
  CloudBest best = {inf, 0x7fffffff};
  if (finite3(a[0], a[1], a[2])) {
    const float lo[3] = {box.lo0, box.lo1, box.lo2};
    const int G[3] = {box.G0, box.G1, box.G2};
    int c[3];
    double A[3];                                                 // the query in the box's frame; h_lo / h_hi: the moved faces' unit
    const double h_lo = (double)box.h * (1.0 + 4e-7), h_hi = (double)box.h * (1.0 - 4e-7);
    int r = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k] = (int)fminf(fmaxf(floorf(__fdiv_rn(__fsub_rn(a[k], lo[k]), box.h)), -kCellFar), kCellFar);
      A[k] = (double)a[k] - (double)lo[k];
      r = max(r, max(-c[k], c[k] - (G[k] - 1)));               // the first ring that touches the grid
    }
    for (;; ++r) {
      // ---- ring r, clipped to the grid: rows on a y or z face of the cube are runs of cells, the others its two x ends -------------
      const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, G[0] - 1);
      const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, G[1] - 1);
      const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, G[2] - 1);
      for (int z = z0; z <= z1; ++z) {
        const bool z_face = z - c[2] == r || c[2] - z == r;
        for (int y = y0; y <= y1; ++y) {
          const int row = (z * G[1] + y) * G[0];
          if (z_face || y - c[1] == r || c[1] - y == r) {
            if (x0 <= x1) scan_run(points, start[row + x0], start[row + x1 + 1], a[0], a[1], a[2], cap2, best);
          } else {
            if (c[0] - r >= 0 && c[0] - r <= G[0] - 1) scan_run(points, start[row + c[0] - r], start[row + c[0] - r + 1], a[0], a[1], a[2], cap2, best);
            if (c[0] + r >= 0 && c[0] + r <= G[0] - 1) scan_run(points, start[row + c[0] + r], start[row + c[0] + r + 1], a[0], a[1], a[2], cap2, best);
          }
        }
      }
      // ---- may the search stop?  The faces of the visited cube with cells behind them: k in 1 .. G - 1 by the choice of the first r --
      double L = std::numeric_limits<double>::infinity();
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int k_lo = c[k] - r, k_hi = c[k] + r + 1;
        if (k_lo >= 1) L = fmin(L, A[k] - (double)k_lo * h_lo);
        if (k_hi <= G[k] - 1) L = fmin(L, (double)k_hi * h_hi - A[k]);
      }
      if (!(L < std::numeric_limits<double>::infinity())) break;              // the rings have left the grid on every side
      if (L > 0.0 && L * L * (1.0 - 1e-6) - 4e-38 > (double)fminf(best.d2, cap2)) break;
    }
  }
  const bool found = best.idx != 0x7fffffff;
  d2_out[q] = found ? best.d2 : inf;
  idx_out[q] = found ? best.idx : -1;
}

// ---- the sums of the scores ----------------------------------------------------------------------------------------------------------
struct CloudTaus {
  float t2[DINER_CLOUD_MAX_THRESHOLDS];
};

// Thread t of workgroup b takes entries b 256 + t, + gridDim.x 256, ... in that order; slot b of the workspace = the workgroup's sums.
__global__ void __launch_bounds__(kCloudThreads) k_cloud_reduce(const float* __restrict__ d2, const int* __restrict__ idx, long long n, float cap2,
                                                                CloudTaus taus, int T, const float* __restrict__ na,
                                                                const float* __restrict__ nb, long long nb_rows, double* __restrict__ ws) {
  __shared__ double red[kCloudWaves];
  double acc[kReduceSlot];
#pragma unroll
  for (int k = 0; k < kReduceSlot; ++k) acc[k] = 0.0;
  const long long stride = (long long)gridDim.x * kCloudThreads;
  for (long long i = blockIdx.x * (long long)kCloudThreads + threadIdx.x; i < n; i += stride) {
    const int j = idx[i];
    const float d = d2[i];
    if (j < 0 || !(d <= cap2)) continue;
    acc[0] += 1.0;
    acc[1] += sqrt((double)d);
    if (na && nb && j < nb_rows) {
      const double dot = ((double)na[3 * i] * (double)nb[3 * (long long)j] + (double)na[3 * i + 1] * (double)nb[3 * (long long)j + 1]) +
                         (double)na[3 * i + 2] * (double)nb[3 * (long long)j + 2];
      acc[2] += fabs(dot);
    }
#pragma unroll
    for (int k = 0; k < DINER_CLOUD_MAX_THRESHOLDS; ++k)
      if (k < T && d <= taus.t2[k]) acc[3 + k] += 1.0;
  }
#pragma unroll
  for (int k = 0; k < kReduceSlot; ++k) {
    const double s = block_sum_d<kCloudWaves>(acc[k], red);
    if (threadIdx.x == 0) ws[(size_t)blockIdx.x * kReduceSlot + k] = s;
  }
}

// One wave: lane l adds slots l, l + 64, ... of each sum, then a fixed xor tree.
__global__ void __launch_bounds__(64) k_cloud_reduce_final(const double* __restrict__ ws, int n_slots, double* __restrict__ out) {
  const int lane = threadIdx.x;
  for (int k = 0; k < kReduceSlot; ++k) {
    double s = 0.0;
    for (int b = lane; b < n_slots; b += 64) s += ws[(size_t)b * kReduceSlot + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[k] = s;
  }
}

int reduce_blocks(long long n) {
  const long long b = (n + kCloudThreads - 1) / kCloudThreads;
  return (int)(b < kReduceBlocks ? b : kReduceBlocks);
}

int check_box(const char* who, const float* lo, float h, int Gx, int Gy, int Gz) {
  DINER_CHECK_ARG(cloud_dims_ok(Gx, Gy, Gz), "%s: grid dims %d x %d x %d (each 1 .. %d, at most 2^26 cells)", who, Gx, Gy, Gz,
                  DINER_CLOUD_MAX_DIM);
  DINER_CHECK_ARG(lo != nullptr, "%s: null pointer argument (lo)", who);
  DINER_CHECK_ARG(std::isfinite(lo[0]) && std::isfinite(lo[1]) && std::isfinite(lo[2]), "%s: box corner lo (%g, %g, %g) is not finite", who,
                  (double)lo[0], (double)lo[1], (double)lo[2]);
  DINER_CHECK_ARG(std::isfinite(h) && h > 0.0f, "%s: cell size %g (need > 0 and finite)", who, (double)h);
  return 0;
}

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" size_t diner_cloud_grid_bytes(long long NB, int Gx, int Gy, int Gz) {
  CloudLayout L;
  return cloud_layout(NB, Gx, Gy, Gz, &L) ? L.bytes : 0;
}

extern "C" size_t diner_cloud_grid_order_offset(long long NB, int Gx, int Gy, int Gz) {
  CloudLayout L;
  return cloud_layout(NB, Gx, Gy, Gz, &L) ? L.order : 0;
}

extern "C" int diner_cloud_grid_build_f32(const float* xyz_b, long long NB, const float* lo, float h, int Gx, int Gy, int Gz, void* workspace,
                                          void* stream) {
  DINER_CHECK_ARG(NB >= 1 && NB <= kCloudMaxPoints, "cloud_grid_build: NB = %lld target points (need 1 .. 2^31 - 1)", NB);
  const int rc = check_box("cloud_grid_build", lo, h, Gx, Gy, Gz);
  if (rc) return rc;
  DINER_CHECK_ARG(xyz_b && workspace, "cloud_grid_build: null pointer argument");
  DINER_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cloud_grid_build: workspace is not 16-byte aligned");
  CloudLayout L;
  cloud_layout(NB, Gx, Gy, Gz, &L);
  char* ws = (char*)workspace;
  int* cursor = (int*)(ws + L.cursor);
  int* start = (int*)(ws + L.start);
  int* tile_sums = (int*)(ws + L.tile_sums);
  const CloudBox box = {lo[0], lo[1], lo[2], h, Gx, Gy, Gz};
  const hipStream_t st = (hipStream_t)stream;
  const long long n = L.cells + 1;
  const unsigned point_blocks = (unsigned)((NB + kCloudThreads - 1) / kCloudThreads);
  DINER_HIP_OK(hipMemsetAsync(cursor, 0, (size_t)n * 4, st));
  hipLaunchKernelGGL(k_cloud_count, dim3(point_blocks), dim3(kCloudThreads), 0, st, xyz_b, (int)NB, box, (int)L.cells, cursor);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_cloud_tile_sums, dim3((unsigned)L.n_tiles), dim3(kCloudThreads), 0, st, (const int*)cursor, n, tile_sums);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_cloud_scan_blocks, dim3(1), dim3(kCloudThreads), 0, st, tile_sums, L.n_tiles);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_cloud_scan_cells, dim3((unsigned)L.n_tiles), dim3(kCloudThreads), 0, st, cursor, n, (const int*)tile_sums, start);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_cloud_scatter, dim3(point_blocks), dim3(kCloudThreads), 0, st, xyz_b, (int)NB, box, (int)L.cells, cursor,
                     (int*)(ws + L.order), (int4*)(ws + L.points));
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_cloud_nearest_f32(const float* xyz_b, long long NB, const float* lo, float h, int Gx, int Gy, int Gz,
                                       const void* workspace, const float* xyz_a, long long NA, const int* order, float max_dist,
                                       float* d2_out, int* idx_out, void* stream) {
  DINER_CHECK_ARG(NB >= 1 && NB <= kCloudMaxPoints, "cloud_nearest: NB = %lld target points (need 1 .. 2^31 - 1)", NB);
  DINER_CHECK_ARG(NA >= 1 && NA <= kCloudMaxPoints, "cloud_nearest: NA = %lld queries (need 1 .. 2^31 - 1)", NA);
  const int rc = check_box("cloud_nearest", lo, h, Gx, Gy, Gz);
  if (rc) return rc;
  DINER_CHECK_ARG(max_dist > 0.0f, "cloud_nearest: max_dist %g (need > 0, or +inf)", (double)max_dist);      // false for a NaN
  DINER_CHECK_ARG(xyz_b && workspace && xyz_a && d2_out && idx_out, "cloud_nearest: null pointer argument");
  DINER_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cloud_nearest: workspace is not 16-byte aligned");
  CloudLayout L;
  cloud_layout(NB, Gx, Gy, Gz, &L);
  const char* ws = (const char*)workspace;
  const CloudBox box = {lo[0], lo[1], lo[2], h, Gx, Gy, Gz};
  const float cap2 = max_dist * max_dist;
  hipLaunchKernelGGL(k_cloud_nearest, dim3((unsigned)((NA + kCloudThreads - 1) / kCloudThreads)), dim3(kCloudThreads), 0, (hipStream_t)stream,
                     (const int*)(ws + L.start), (const int4*)(ws + L.points), box, xyz_a, (int)NA, order, cap2, d2_out, idx_out);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" size_t diner_cloud_reduce_workspace_bytes(long long n) {
  if (n < 1) return 0;
  return (size_t)reduce_blocks(n) * kReduceSlot * sizeof(double);
}

extern "C" int diner_cloud_reduce_f32(const float* d2, const int* idx, long long n, float max_dist, const float* thresholds, int T,
                                      const float* normals_a, const float* normals_b, long long nb_rows, void* workspace, double* out,
                                      void* stream) {
  DINER_CHECK_ARG(n >= 1, "cloud_reduce: n = %lld entries (need >= 1)", n);
  DINER_CHECK_ARG(max_dist > 0.0f, "cloud_reduce: max_dist %g (need > 0, or +inf)", (double)max_dist);
  DINER_CHECK_ARG(T >= 0 && T <= DINER_CLOUD_MAX_THRESHOLDS, "cloud_reduce: T = %d thresholds (need 0 .. %d)", T, DINER_CLOUD_MAX_THRESHOLDS);
  DINER_CHECK_ARG(T == 0 || thresholds != nullptr, "cloud_reduce: null pointer argument (thresholds)");
  CloudTaus taus;
  memset(&taus, 0, sizeof(taus));
  for (int k = 0; k < T; ++k) {
    DINER_CHECK_ARG(thresholds[k] >= 0.0f, "cloud_reduce: threshold %d is %g (need >= 0)", k, (double)thresholds[k]);
    taus.t2[k] = thresholds[k] * thresholds[k];
  }
  DINER_CHECK_ARG(d2 && idx && workspace && out, "cloud_reduce: null pointer argument");
  DINER_CHECK_ARG((normals_a == nullptr) == (normals_b == nullptr), "cloud_reduce: normals_a and normals_b go together");
  DINER_CHECK_ARG(normals_b == nullptr || nb_rows >= 1, "cloud_reduce: nb_rows = %lld rows of normals_b (need >= 1)", nb_rows);
  const int blocks = reduce_blocks(n);
  hipLaunchKernelGGL(k_cloud_reduce, dim3((unsigned)blocks), dim3(kCloudThreads), 0, (hipStream_t)stream, d2, idx, n, max_dist * max_dist, taus,
                     T, normals_a, normals_b, nb_rows, (double*)workspace);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_cloud_reduce_final, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, blocks, out);
  DINER_LAUNCH_OK();
  return 0;
}
