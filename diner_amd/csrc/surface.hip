// Surfaces from depth maps: fuse N z-depth maps into a truncated signed distance volume (Curless & Levoy) and pull an indexed,
// oriented triangle mesh out of it with naive surface nets.
//
// The volume is an axis-aligned box: sample (i, j, k) lies at origin + (i, j, k) voxel; the device planes are (Nz, Ny, Nx) fp32, x
// fastest: tsdf (fresh = 1), wsum (fresh = 0) and optionally color4 (4, Nz, Ny, Nx) = sum w r, sum w g, sum w b, sum w (fresh = 0).
//
// diner_tsdf_integrate_f32: one thread per voxel; the voxel's tsdf / wsum / colour sums live in registers across a loop over the views
// IN VIEW ORDER, so the volume is read and written once per call whatever N, and one call with N views leaves the bits of N single-view
// calls.  The cameras travel as kernel arguments (16 floats a view, 1 KiB), as in k_depth_consistency.
//
// diner_surface_count / diner_surface_extract_f32: one thread per grid sample v = (i, j, k), which owns the cell whose lowest corner it
// is and the three grid edges that start at it.  Four launches ordered by the stream alone (no workgroup waits on another, no atomics):
// vertices and quads per block of kSurfThreads samples -> one workgroup scans the block counts -> every block scans its own flags
// again, writes its vertices and the cell -> vertex map -> every block writes the faces of its edges through that map.  Topology is
// decided by exact comparisons only (tsdf < 0, wsum > min_weight): counts, ids and faces are a function of the volume's bits.
#include "common.hpp"

namespace diner {

namespace {

constexpr int kSurfThreads = 256;                 // grid samples per workgroup of the count / vertex / face kernels
constexpr int kSurfHeaderInts = 4;                // workspace: [0] vertices, [1] quads as count wrote them, [2..3] unused
constexpr int kSurfMaxDim = 1024;

// ---- integration ---------------------------------------------------------------------------------------------------------------
struct TsdfCam {        // R (world->cam, row-major), t, fx, fy, cx, cy
  float R[9], t[3], fx, fy, cx, cy;
};
struct TsdfCams {
  TsdfCam cam[kMaxViewsWide];
};

__global__ __launch_bounds__(256) void k_tsdf_integrate(float* __restrict__ tsdf, float* __restrict__ wsum, float* __restrict__ color4,
                                                        int Nx, int Ny, long long n_vox, float o0, float o1, float o2, float voxel,
                                                        float trunc, const float* __restrict__ depth, const float* __restrict__ weight,
                                                        const float* __restrict__ color, TsdfCams cams, int N, int H, int W, int carve,
                                                        float max_weight) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= n_vox) return;
  const unsigned row = (unsigned)idx / (unsigned)Nx;                    // n_vox < 2^31: 32-bit divisions
  const int i = (int)((unsigned)idx - row * (unsigned)Nx);
  const int k = (int)(row / (unsigned)Ny), j = (int)(row - (unsigned)k * (unsigned)Ny);
  const float p0 = __fadd_rn(o0, __fmul_rn((float)i, voxel));
  const float p1 = __fadd_rn(o1, __fmul_rn((float)j, voxel));
  const float p2 = __fadd_rn(o2, __fmul_rn((float)k, voxel));
  float f = tsdf[idx], ws = wsum[idx];
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
  if (color4) {
    c0 = color4[idx];
    c1 = color4[(size_t)n_vox + idx];
    c2 = color4[(size_t)n_vox * 2 + idx];
    c3 = color4[(size_t)n_vox * 3 + idx];
  }
  const size_t HW = (size_t)H * W;
  // A view that does not see the voxel costs no load: the skips are branches on purpose.  (Measured: a branch-free body that loads
  // every view's depth, weight and colour at a clamped address and selects afterwards takes 6.3 ms where this takes 1.2 ms on sixteen
  // 800 x 600 views and a 256^3 volume -- the colour taps of the few voxels near a surface became taps of every voxel.)
  for (int n = 0; n < N; ++n) {
    const TsdfCam& c = cams.cam[n];
    const float x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.R[0], p0), __fmul_rn(c.R[1], p1)), __fmul_rn(c.R[2], p2)), c.t[0]);
    const float y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.R[3], p0), __fmul_rn(c.R[4], p1)), __fmul_rn(c.R[5], p2)), c.t[1]);
    const float z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.R[6], p0), __fmul_rn(c.R[7], p1)), __fmul_rn(c.R[8], p2)), c.t[2]);
    if (!(z > 0.0f)) continue;                                         // behind the camera (or NaN)
    const float u = __fadd_rn(__fmul_rn(c.fx, __fdiv_rn(x, z)), c.cx);
    const float v = __fadd_rn(__fmul_rn(c.fy, __fdiv_rn(y, z)), c.cy);
    if (!(u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H)) continue;     // outside the image (or NaN)
    const int pj = (int)u, pi = (int)v;                                // floor: both are >= 0; pj <= W - 1, pi <= H - 1
    const size_t pix = (size_t)n * HW + (size_t)pi * W + pj;
    const float wp = weight ? weight[pix] : 1.0f;
    if (!(wp > 0.0f)) continue;
    const float D = depth[pix];
    float d;
    bool paint = false;
    if (D > 0.0f) {
      const float sdf = __fsub_rn(D, z);
      if (sdf < -trunc) continue;                                      // hidden behind the surface
      d = fminf(1.0f, __fdiv_rn(sdf, trunc));
      paint = sdf <= trunc;
    } else if (D == 0.0f && carve) {
      d = 1.0f;                                                        // the pixel is empty: the whole ray is free space
    } else {
      continue;                                                        // no surface and no carving, a negative depth, a NaN
    }
    const float wn = __fadd_rn(ws, wp);
    f = __fdiv_rn(__fadd_rn(__fmul_rn(f, ws), __fmul_rn(d, wp)), wn);
    ws = max_weight > 0.0f ? fminf(wn, max_weight) : wn;
    if (color4 && paint) {
      const float* cp = color + (size_t)n * 3 * HW + (size_t)pi * W + pj;
      c0 = __fadd_rn(c0, __fmul_rn(wp, cp[0]));
      c1 = __fadd_rn(c1, __fmul_rn(wp, cp[HW]));
      c2 = __fadd_rn(c2, __fmul_rn(wp, cp[2 * HW]));
      c3 = __fadd_rn(c3, wp);
    }
  }
  tsdf[idx] = f;
  wsum[idx] = ws;
  if (color4) {
    color4[idx] = c0;
    color4[(size_t)n_vox + idx] = c1;
    color4[(size_t)n_vox * 2 + idx] = c2;
    color4[(size_t)n_vox * 3 + idx] = c3;
  }
}

// ---- surface nets ----------------------------------------------------------------------------------------------------------------
struct SurfGrid {
  const float* tsdf;
  const float* wsum;
  int Nx, Ny, Nz;
  long long n_vox;
  float min_weight;
};

__device__ __forceinline__ long long vox(const SurfGrid& g, int i, int j, int k) { return ((long long)k * g.Ny + j) * g.Nx + i; }

// Cell (i, j, k): exists iff 0 <= i < Nx - 1 (and so on); active iff all 8 corners are observed and both signs occur.
__device__ __forceinline__ bool cell_active(const SurfGrid& g, int i, int j, int k) {
  if (i < 0 || j < 0 || k < 0 || i >= g.Nx - 1 || j >= g.Ny - 1 || k >= g.Nz - 1) return false;
  int n_neg = 0;
  bool seen = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const long long v = vox(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));
    n_neg += g.tsdf[v] < 0.0f ? 1 : 0;
    seen = seen && g.wsum[v] > g.min_weight;
  }
  return seen && n_neg > 0 && n_neg < 8;
}

// The grid edge from (i, j, k) along `axis` (0: +x, 1: +y, 2: +z) emits a quad iff it exists, changes sign and its four cells are active.
// -> 0: none, 1: the start is negative (the quad's normal points along +axis), 2: the start is positive.
__device__ __forceinline__ int edge_quad(const SurfGrid& g, int i, int j, int k, int axis) {
  const int ei = i + (axis == 0), ej = j + (axis == 1), ek = k + (axis == 2);
  if (ei >= g.Nx || ej >= g.Ny || ek >= g.Nz) return 0;
  const bool na = g.tsdf[vox(g, i, j, k)] < 0.0f, nb = g.tsdf[vox(g, ei, ej, ek)] < 0.0f;
  if (na == nb) return 0;
  // the other two axes in cyclic order: u x v = axis
  const int ua = (axis + 1) % 3, va = (axis + 2) % 3;
  const int du[3] = {ua == 0, ua == 1, ua == 2}, dv[3] = {va == 0, va == 1, va == 2};
  const bool all = cell_active(g, i - du[0] - dv[0], j - du[1] - dv[1], k - du[2] - dv[2]) &&
                   cell_active(g, i - dv[0], j - dv[1], k - dv[2]) && cell_active(g, i, j, k) &&
                   cell_active(g, i - du[0], j - du[1], k - du[2]);
  return all ? (na ? 1 : 2) : 0;
}

// Inclusive sum over the workgroup in thread order; `red` (WAVES ints) is reused by the next call after its trailing barrier.
template <int WAVES>
__device__ __forceinline__ int surf_scan_incl(int v, int* red, int* total) {
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
  for (int w = 0; w < WAVES; ++w) {
    const int c = red[w];
    if (w < wave) before += c;
    all += c;
  }
  __syncthreads();
  *total = all;
  return v + before;
}

constexpr int kSurfWaves = kSurfThreads / kWave;

// What the sample's thread owns: 1 vertex if its cell is active, and up to 3 quads.
__device__ __forceinline__ void sample_counts(const SurfGrid& g, long long v, int& i, int& j, int& k, int& n_vert, int q[3]) {
  n_vert = 0;
  q[0] = q[1] = q[2] = 0;
  i = j = k = 0;
  if (v >= g.n_vox) return;
  const unsigned row = (unsigned)v / (unsigned)g.Nx;                    // n_vox < 2^31: 32-bit divisions
  i = (int)((unsigned)v - row * (unsigned)g.Nx);
  k = (int)(row / (unsigned)g.Ny);
  j = (int)(row - (unsigned)k * (unsigned)g.Ny);
  n_vert = cell_active(g, i, j, k) ? 1 : 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = edge_quad(g, i, j, k, a);
}

__global__ void __launch_bounds__(kSurfThreads) k_surf_count(SurfGrid g, int* __restrict__ block_counts) {
  __shared__ int red[kSurfWaves];
  const long long v = blockIdx.x * (long long)kSurfThreads + threadIdx.x;
  int i, j, k, n_vert, q[3];
  sample_counts(g, v, i, j, k, n_vert, q);
  int tv, tq;
  surf_scan_incl<kSurfWaves>(n_vert, red, &tv);
  surf_scan_incl<kSurfWaves>((q[0] != 0) + (q[1] != 0) + (q[2] != 0), red, &tq);
  if (threadIdx.x == 0) {
    block_counts[2 * (size_t)blockIdx.x] = tv;
    block_counts[2 * (size_t)blockIdx.x + 1] = tq;
  }
}

// One workgroup: block_counts[b] -> the id of block b's first vertex / quad, kSurfThreads blocks a pass; the totals go to the workspace
// header and to counts_out.
__global__ void __launch_bounds__(kSurfThreads) k_surf_scan(int* __restrict__ block_counts, long long n_blocks, int* __restrict__ header,
                                                            int* __restrict__ counts_out) {
  __shared__ int red[kSurfWaves];
  int carry_v = 0, carry_q = 0;
  for (long long b0 = 0; b0 < n_blocks; b0 += kSurfThreads) {
    const long long b = b0 + threadIdx.x;
    const int cv = b < n_blocks ? block_counts[2 * b] : 0;
    const int cq = b < n_blocks ? block_counts[2 * b + 1] : 0;
    int tv, tq;
    const int iv = surf_scan_incl<kSurfWaves>(cv, red, &tv);
    const int iq = surf_scan_incl<kSurfWaves>(cq, red, &tq);
    if (b < n_blocks) {
      block_counts[2 * b] = carry_v + iv - cv;
      block_counts[2 * b + 1] = carry_q + iq - cq;
    }
    carry_v += tv;
    carry_q += tq;
  }
  if (threadIdx.x == 0) {
    header[0] = carry_v;
    header[1] = carry_q;
    counts_out[0] = carry_v;
    counts_out[1] = carry_q;
  }
}

__device__ __forceinline__ float lerp_rn(float a, float b, float t) {
  return __fadd_rn(__fmul_rn(a, __fsub_rn(1.0f, t)), __fmul_rn(b, t));
}
// corners f[c], c = x + 2 y + 4 z: along x, then y, then z
__device__ __forceinline__ float trilinear(const float f[8], float mx, float my, float mz) {
  const float a0 = lerp_rn(f[0], f[1], mx), a1 = lerp_rn(f[2], f[3], mx), a2 = lerp_rn(f[4], f[5], mx), a3 = lerp_rn(f[6], f[7], mx);
  return lerp_rn(lerp_rn(a0, a1, my), lerp_rn(a2, a3, my), mz);
}
// d/d(axis) of the trilinear interpolant: the four differences along the axis, bilinear in the other two (p then q)
__device__ __forceinline__ float bilinear4(float d00, float d10, float d01, float d11, float p, float q) {
  return lerp_rn(lerp_rn(d00, d10, p), lerp_rn(d01, d11, p), q);
}

struct SurfOut {
  float* vertices;
  float* normals;
  float* rgb;
};

__global__ void __launch_bounds__(kSurfThreads) k_surf_vertices(SurfGrid g, const float* __restrict__ color4, float o0, float o1, float o2,
                                                                float voxel, const int* __restrict__ block_offsets, int n_vertices,
                                                                int* __restrict__ cell_vertex, SurfOut out) {
  __shared__ int red[kSurfWaves];
  const long long v = blockIdx.x * (long long)kSurfThreads + threadIdx.x;
  int i = 0, j = 0, k = 0, active = 0;
  if (v < g.n_vox) {
    const unsigned row = (unsigned)v / (unsigned)g.Nx;                  // n_vox < 2^31: 32-bit divisions
    i = (int)((unsigned)v - row * (unsigned)g.Nx);
    k = (int)(row / (unsigned)g.Ny);
    j = (int)(row - (unsigned)k * (unsigned)g.Ny);
    active = cell_active(g, i, j, k) ? 1 : 0;
  }
  int total;
  const int incl = surf_scan_incl<kSurfWaves>(active, red, &total);   // the last barrier of the kernel: returns below are free
  if (v >= g.n_vox) return;
  const long long id64 = (long long)block_offsets[2 * (size_t)blockIdx.x] + incl - active;
  const bool write = active && id64 >= 0 && id64 < n_vertices;        // an id outside the caller's arrays is not written
  cell_vertex[v] = write ? (int)id64 : -1;
  if (!write) return;
  const int id = (int)id64;
  float f[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) f[c] = g.tsdf[vox(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))];
  // mean over the sign-changing cell edges of a + t (b - a), t = f_a / (f_a - f_b): the four x-edges, then y, then z, each in corner order
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  int n_edges = 0;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    const int step = 1 << axis;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      if (a & step) continue;
      const float fa = f[a], fb = f[a + step];
      if ((fa < 0.0f) == (fb < 0.0f)) continue;
      const float t = __fdiv_rn(fa, __fsub_rn(fa, fb));
      sx = __fadd_rn(sx, axis == 0 ? t : (float)(a & 1));
      sy = __fadd_rn(sy, axis == 1 ? t : (float)((a >> 1) & 1));
      sz = __fadd_rn(sz, axis == 2 ? t : (float)(a >> 2));
      ++n_edges;
    }
  }
  const float ne = (float)n_edges;                                     // >= 3: both signs occur among the corners
  const float mx = __fdiv_rn(sx, ne), my = __fdiv_rn(sy, ne), mz = __fdiv_rn(sz, ne);
  float* vp = out.vertices + (size_t)id * 3;
  vp[0] = __fadd_rn(o0, __fmul_rn(voxel, __fadd_rn((float)i, mx)));
  vp[1] = __fadd_rn(o1, __fmul_rn(voxel, __fadd_rn((float)j, my)));
  vp[2] = __fadd_rn(o2, __fmul_rn(voxel, __fadd_rn((float)k, mz)));
  if (out.normals) {
    const float gx = bilinear4(__fsub_rn(f[1], f[0]), __fsub_rn(f[3], f[2]), __fsub_rn(f[5], f[4]), __fsub_rn(f[7], f[6]), my, mz);
    const float gy = bilinear4(__fsub_rn(f[2], f[0]), __fsub_rn(f[3], f[1]), __fsub_rn(f[6], f[4]), __fsub_rn(f[7], f[5]), mx, mz);
    const float gz = bilinear4(__fsub_rn(f[4], f[0]), __fsub_rn(f[5], f[1]), __fsub_rn(f[6], f[2]), __fsub_rn(f[7], f[3]), mx, my);
    const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), __fmul_rn(gz, gz)));
    const bool ok = len > 0.0f;                                        // false for a NaN
    float* np = out.normals + (size_t)id * 3;
    np[0] = ok ? __fdiv_rn(gx, len) : 0.0f;
    np[1] = ok ? __fdiv_rn(gy, len) : 0.0f;
    np[2] = ok ? __fdiv_rn(gz, len) : 0.0f;
  }
  if (out.rgb) {
    float* cp = out.rgb + (size_t)id * 3;
    float den = 0.0f;
    if (color4) {
#pragma unroll
      for (int c = 0; c < 8; ++c) f[c] = color4[(size_t)g.n_vox * 3 + vox(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))];
      den = trilinear(f, mx, my, mz);
    }
    const bool ok = den > 0.0f;
    for (int ch = 0; ch < 3; ++ch) {
      float val = 0.0f;
      if (ok) {
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] = color4[(size_t)g.n_vox * ch + vox(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))];
        val = __fdiv_rn(trilinear(f, mx, my, mz), den);
      }
      cp[ch] = val;
    }
  }
}

__global__ void __launch_bounds__(kSurfThreads) k_surf_faces(SurfGrid g, const int* __restrict__ block_offsets,
                                                             const int* __restrict__ cell_vertex, int n_quads, int* __restrict__ faces) {
  __shared__ int red[kSurfWaves];
  const long long v = blockIdx.x * (long long)kSurfThreads + threadIdx.x;
  int i, j, k, n_vert, q[3];
  sample_counts(g, v, i, j, k, n_vert, q);
  const int mine = (q[0] != 0) + (q[1] != 0) + (q[2] != 0);
  int total;
  const int incl = surf_scan_incl<kSurfWaves>(mine, red, &total);     // the last barrier of the kernel
  if (mine == 0) return;
  long long qid = (long long)block_offsets[2 * (size_t)blockIdx.x + 1] + incl - mine;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    if (q[axis] == 0) continue;
    if (qid >= 0 && qid < n_quads) {
      const int ua = (axis + 1) % 3, va = (axis + 2) % 3;
      const int du[3] = {ua == 0, ua == 1, ua == 2}, dv[3] = {va == 0, va == 1, va == 2};
      // the four cells round the edge, counter-clockwise seen from +axis, from the one with the smallest indices
      const int v0 = cell_vertex[vox(g, i - du[0] - dv[0], j - du[1] - dv[1], k - du[2] - dv[2])];
      const int v1 = cell_vertex[vox(g, i - dv[0], j - dv[1], k - dv[2])];
      const int v2 = cell_vertex[v];
      const int v3 = cell_vertex[vox(g, i - du[0], j - du[1], k - du[2])];
      const int a = q[axis] == 1 ? v1 : v3, c = q[axis] == 1 ? v3 : v1;       // a positive start turns the quad round
      int* fp = faces + (size_t)qid * 6;
      fp[0] = v0; fp[1] = a; fp[2] = v2;
      fp[3] = v0; fp[4] = v2; fp[5] = c;
    }
    ++qid;
  }
}

bool dims_ok(int Nx, int Ny, int Nz) {
  return Nx >= 2 && Ny >= 2 && Nz >= 2 && Nx <= kSurfMaxDim && Ny <= kSurfMaxDim && Nz <= kSurfMaxDim &&
         (long long)Nx * Ny * Nz <= 0x7fffffffLL;
}
long long surf_blocks(int Nx, int Ny, int Nz) { return ((long long)Nx * Ny * Nz + kSurfThreads - 1) / kSurfThreads; }

struct SurfWorkspace {
  int* header;
  int* block_counts;
  int* cell_vertex;
};
SurfWorkspace split_workspace(void* workspace, int Nx, int Ny, int Nz) {
  int* base = static_cast<int*>(workspace);
  return {base, base + kSurfHeaderInts, base + kSurfHeaderInts + 2 * surf_blocks(Nx, Ny, Nz)};
}

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" int diner_tsdf_integrate_f32(float* tsdf, float* wsum, float* color4, int Nx, int Ny, int Nz, const float* origin, float voxel,
                                        float trunc, const float* depth, const float* weight, const float* color,
                                        const float* intrinsics, const float* extrinsics, int N, int H, int W, int carve,
                                        float max_weight, void* stream) {
  DINER_CHECK_ARG(N >= 1 && N <= kMaxViewsWide, "tsdf_integrate: %d views outside [1, %d]", N, kMaxViewsWide);
  DINER_CHECK_ARG(dims_ok(Nx, Ny, Nz), "tsdf_integrate: volume dimension %d x %d x %d (each 2 .. %d, fewer than 2^31 samples)", Nx, Ny, Nz,
                  kSurfMaxDim);
  DINER_CHECK_ARG(voxel > 0.0f, "tsdf_integrate: voxel size %g (need > 0)", (double)voxel);
  DINER_CHECK_ARG(trunc > 0.0f, "tsdf_integrate: truncation distance %g (need > 0)", (double)trunc);
  DINER_CHECK_ARG((color != nullptr) == (color4 != nullptr), "tsdf_integrate: color maps and the color4 planes come together");
  DINER_CHECK_ARG(tsdf && wsum && origin && depth && intrinsics && extrinsics, "tsdf_integrate: null pointer argument");
  DINER_CHECK_ARG(H >= 1 && W >= 1 && (long long)N * 3 * H * W <= 0x7fffffffLL, "tsdf_integrate: bad map size %d x %d x %d", N, H, W);
  DINER_CHECK_ARG(max_weight == max_weight, "tsdf_integrate: max_weight is NaN");
  TsdfCams cams;
  memset(&cams, 0, sizeof(cams));
  for (int n = 0; n < N; ++n) {
    const float* E = extrinsics + 16 * n;
    const float* Kn = intrinsics + 9 * n;
    TsdfCam& c = cams.cam[n];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) c.R[3 * a + b] = E[4 * a + b];
      c.t[a] = E[4 * a + 3];
    }
    c.fx = Kn[0];
    c.fy = Kn[4];
    c.cx = Kn[2];
    c.cy = Kn[5];
  }
  const long long n_vox = (long long)Nx * Ny * Nz;
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tsdf, wsum, color4, Nx, Ny,
                     n_vox, origin[0], origin[1], origin[2], voxel, trunc, depth, weight, color, cams, N, H, W, carve, max_weight);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" size_t diner_surface_workspace_bytes(int Nx, int Ny, int Nz) {
  if (!dims_ok(Nx, Ny, Nz)) return 0;
  return sizeof(int) * (size_t)(kSurfHeaderInts + 2 * surf_blocks(Nx, Ny, Nz) + (long long)Nx * Ny * Nz);
}

extern "C" int diner_surface_count(const float* tsdf, const float* wsum, int Nx, int Ny, int Nz, float min_weight, void* workspace,
                                   int* counts_out, void* stream) {
  DINER_CHECK_ARG(dims_ok(Nx, Ny, Nz), "surface_count: volume dimension %d x %d x %d (each 2 .. %d, fewer than 2^31 samples)", Nx, Ny, Nz,
                  kSurfMaxDim);
  DINER_CHECK_ARG(tsdf && wsum && workspace && counts_out, "surface_count: null pointer argument");
  DINER_CHECK_ARG(min_weight == min_weight, "surface_count: min_weight is NaN");
  hipStream_t st = (hipStream_t)stream;
  const SurfWorkspace ws = split_workspace(workspace, Nx, Ny, Nz);
  const long long n_blocks = surf_blocks(Nx, Ny, Nz);
  const SurfGrid g = {tsdf, wsum, Nx, Ny, Nz, (long long)Nx * Ny * Nz, min_weight};
  hipLaunchKernelGGL(k_surf_count, dim3((unsigned)n_blocks), dim3(kSurfThreads), 0, st, g, ws.block_counts);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_surf_scan, dim3(1), dim3(kSurfThreads), 0, st, ws.block_counts, n_blocks, ws.header, counts_out);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_surface_extract_f32(const float* tsdf, const float* wsum, const float* color4, int Nx, int Ny, int Nz,
                                         const float* origin, float voxel, float min_weight, void* workspace, int n_vertices, int n_quads,
                                         float* vertices_out, float* normals_out, float* rgb_out, int* faces_out, void* stream) {
  DINER_CHECK_ARG(dims_ok(Nx, Ny, Nz), "surface_extract: volume dimension %d x %d x %d (each 2 .. %d, fewer than 2^31 samples)", Nx, Ny,
                  Nz, kSurfMaxDim);
  DINER_CHECK_ARG(voxel > 0.0f, "surface_extract: voxel size %g (need > 0)", (double)voxel);
  DINER_CHECK_ARG(tsdf && wsum && origin && workspace, "surface_extract: null pointer argument");
  DINER_CHECK_ARG(min_weight == min_weight, "surface_extract: min_weight is NaN");
  DINER_CHECK_ARG(n_vertices >= 0 && n_quads >= 0, "surface_extract: counts %d, %d (need >= 0)", n_vertices, n_quads);
  DINER_CHECK_ARG(n_vertices == 0 || vertices_out, "surface_extract: %d vertices without an output array", n_vertices);
  DINER_CHECK_ARG(n_quads == 0 || faces_out, "surface_extract: %d quads without an output array", n_quads);
  hipStream_t st = (hipStream_t)stream;
  const SurfWorkspace ws = split_workspace(workspace, Nx, Ny, Nz);
  // the counts must be the ones diner_surface_count left in the workspace: one 8-byte read, the entry's only host synchronisation
  int seen[2] = {-1, -1};
  DINER_HIP_OK(hipMemcpyAsync(seen, ws.header, sizeof(seen), hipMemcpyDeviceToHost, st));
  DINER_HIP_OK(hipStreamSynchronize(st));
  DINER_CHECK_ARG(seen[0] == n_vertices && seen[1] == n_quads, "surface_extract: counts %d, %d are not the %d, %d surface_count wrote",
                  n_vertices, n_quads, seen[0], seen[1]);
  if (n_vertices == 0) return 0;                                       // no vertex, hence no quad
  const long long n_blocks = surf_blocks(Nx, Ny, Nz);
  const SurfGrid g = {tsdf, wsum, Nx, Ny, Nz, (long long)Nx * Ny * Nz, min_weight};
  const SurfOut out = {vertices_out, normals_out, rgb_out};
  hipLaunchKernelGGL(k_surf_vertices, dim3((unsigned)n_blocks), dim3(kSurfThreads), 0, st, g, color4, origin[0], origin[1], origin[2], voxel,
                     (const int*)ws.block_counts, n_vertices, ws.cell_vertex, out);
  DINER_LAUNCH_OK();
  if (n_quads > 0) {
    hipLaunchKernelGGL(k_surf_faces, dim3((unsigned)n_blocks), dim3(kSurfThreads), 0, st, g, (const int*)ws.block_counts,
                       (const int*)ws.cell_vertex, n_quads, faces_out);
    DINER_LAUNCH_OK();
  }
  return 0;
}
