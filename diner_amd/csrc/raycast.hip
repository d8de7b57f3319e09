// Ray-cast a TSDF volume (surface.hip's planes and conventions) into z-depth, camera-facing normals, colour and confidence maps of any
// cameras: the volume seen as an image, KinectFusion's second half.
//
// k_tsdf_raycast: one thread per ray, a wavefront covers an 8 x 8 pixel tile (four tiles, 16 x 16 pixels, a workgroup), so neighbouring
// rays walk the same cells and the 8-tap gathers of a wave fall on few cache lines.  No LDS, no atomics, no barrier.  The samples sit on
// a lattice anchored at the camera, z_n = n dz, each a product and each evaluated from its own n: where a thread starts, what it jumps
// over and where it stops change which samples are LOOKED AT, never what a sample IS, so the outputs with and without the brick mask
// are the same bits.  The loop is bounded by a trip count the host computes; no ray can spin.
//
// k_tsdf_bricks: one wavefront per brick of 8^3 cells, one byte each: 1 iff some cell of the brick has all 8 corners observed and a
// negative corner.  A lattice sample whose cell lies in a 0-brick cannot be observed and negative, so it cannot end a march.
#include "common.hpp"

#include <cmath>

namespace diner {

namespace {

constexpr int kCastMaxDim = 1024;
constexpr int kCastTile = 16;                      // pixels a side of a workgroup: 2 x 2 wavefronts of 8 x 8 pixels
constexpr long long kCastMaxSamples = 1 << 20;     // lattice samples a ray may have
constexpr int kBrick = 8;                          // cells a side of a brick

struct CastCam {        // R (world->cam, row-major), t, fx, fy, cx, cy
  float R[9], t[3], fx, fy, cx, cy;
};
struct CastCams {
  CastCam cam[kMaxViewsWide];
};

struct CastVolume {
  const float* tsdf;
  const float* wsum;
  const float* color4;
  const unsigned char* bricks;
  int Nx, Ny, Nz;
  float o0, o1, o2, voxel, min_weight;
};

struct CastOut {
  float* zdepth;
  float* normal;
  float* rgb;
  float* weight;
};

// Square roots are sqrtf, which hipcc rounds correctly by default; __fsqrt_rn is the hardware's approximate v_sqrt_f32 in this build.
__device__ __forceinline__ float lerp_ab(float a, float b, float w) { return __fadd_rn(a, __fmul_rn(w, __fsub_rn(b, a))); }
// corners f[c], c = x + 2 y + 4 z: along x, then y, then z
__device__ __forceinline__ float trilinear_ab(const float f[8], float mx, float my, float mz) {
  const float a0 = lerp_ab(f[0], f[1], mx), a1 = lerp_ab(f[2], f[3], mx), a2 = lerp_ab(f[4], f[5], mx), a3 = lerp_ab(f[6], f[7], mx);
  return lerp_ab(lerp_ab(a0, a1, my), lerp_ab(a2, a3, my), mz);
}
// d/d(axis) of the trilinear interpolant: the four differences along the axis, bilinear in the other two (p then q)
__device__ __forceinline__ float bilinear_ab(float d00, float d10, float d01, float d11, float p, float q) {
  return lerp_ab(lerp_ab(d00, d10, p), lerp_ab(d01, d11, p), q);
}

struct CastRay {
  float e0, e1, e2, d0, d1, d2;                    // eye and d_w
};

// The grid position of p(z), its cell (clamped to the volume: every load below is in bounds whatever z) and the fraction in the cell.
struct CastCell {
  float g0, g1, g2, m0, m1, m2;
  int i, j, k;
};
__device__ __forceinline__ CastCell cell_at(const CastVolume& v, const CastRay& r, float z) {
  CastCell c;
  c.g0 = __fdiv_rn(__fsub_rn(__fadd_rn(r.e0, __fmul_rn(z, r.d0)), v.o0), v.voxel);
  c.g1 = __fdiv_rn(__fsub_rn(__fadd_rn(r.e1, __fmul_rn(z, r.d1)), v.o1), v.voxel);
  c.g2 = __fdiv_rn(__fsub_rn(__fadd_rn(r.e2, __fmul_rn(z, r.d2)), v.o2), v.voxel);
  const float f0 = fminf(fmaxf(floorf(c.g0), 0.0f), (float)(v.Nx - 2));     // fmaxf / fminf drop a NaN: the cell is then 0
  const float f1 = fminf(fmaxf(floorf(c.g1), 0.0f), (float)(v.Ny - 2));
  const float f2 = fminf(fmaxf(floorf(c.g2), 0.0f), (float)(v.Nz - 2));
  c.i = (int)f0;
  c.j = (int)f1;
  c.k = (int)f2;
  c.m0 = __fsub_rn(c.g0, f0);
  c.m1 = __fsub_rn(c.g1, f1);
  c.m2 = __fsub_rn(c.g2, f2);
  return c;
}
__device__ __forceinline__ bool inside(const CastVolume& v, const CastCell& c) {
  return c.g0 >= 0.0f && c.g0 <= (float)(v.Nx - 1) && c.g1 >= 0.0f && c.g1 <= (float)(v.Ny - 1) && c.g2 >= 0.0f &&
         c.g2 <= (float)(v.Nz - 1);
}
__device__ __forceinline__ void gather8(const float* __restrict__ plane, const CastVolume& v, const CastCell& c, float f[8]) {
  const float* p = plane + ((size_t)c.k * v.Ny + c.j) * v.Nx + c.i;
  const size_t sy = (size_t)v.Nx, sz = (size_t)v.Nx * v.Ny;
#pragma unroll
  for (int q = 0; q < 8; ++q) f[q] = p[(q & 1) + ((q >> 1) & 1) * sy + (q >> 2) * sz];
}
// Lattice sample at camera depth z: observed iff inside, z >= znear and the 8 corners of its cell are observed; *f = the interpolant.
__device__ __forceinline__ bool sample_at(const CastVolume& v, const CastRay& r, float z, float znear, float* f) {
  const CastCell c = cell_at(v, r, z);
  if (!(inside(v, c) && z >= znear)) return false;
  float w[8], t[8];
  gather8(v.wsum, v, c, w);
  gather8(v.tsdf, v, c, t);
  bool seen = true;
#pragma unroll
  for (int q = 0; q < 8; ++q) seen = seen && w[q] > v.min_weight;
  *f = trilinear_ab(t, c.m0, c.m1, c.m2);
  return seen;
}

__global__ __launch_bounds__(256) void k_tsdf_raycast(CastVolume v, CastCams cams, int H, int W, float znear, float zfar, float step,
                                                      int n_max, CastOut out) {
  // wavefront w of the workgroup owns the 8 x 8 tile (w & 1, w >> 1) of its 16 x 16 pixels
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int c = blockIdx.x * kCastTile + (wave & 1) * 8 + (lane & 7);
  const int r = blockIdx.y * kCastTile + (wave >> 1) * 8 + (lane >> 3);
  const int view = blockIdx.z;
  if (c >= W || r >= H) return;
  const CastCam& cam = cams.cam[view];
  const float* R = cam.R;
  CastRay ray;
  ray.e0 = -__fadd_rn(__fadd_rn(__fmul_rn(R[0], cam.t[0]), __fmul_rn(R[3], cam.t[1])), __fmul_rn(R[6], cam.t[2]));
  ray.e1 = -__fadd_rn(__fadd_rn(__fmul_rn(R[1], cam.t[0]), __fmul_rn(R[4], cam.t[1])), __fmul_rn(R[7], cam.t[2]));
  ray.e2 = -__fadd_rn(__fadd_rn(__fmul_rn(R[2], cam.t[0]), __fmul_rn(R[5], cam.t[1])), __fmul_rn(R[8], cam.t[2]));
  const float dcx = __fdiv_rn(__fsub_rn(__fadd_rn((float)c, 0.5f), cam.cx), cam.fx);
  const float dcy = __fdiv_rn(__fsub_rn(__fadd_rn((float)r, 0.5f), cam.cy), cam.fy);
  ray.d0 = __fadd_rn(__fadd_rn(__fmul_rn(R[0], dcx), __fmul_rn(R[3], dcy)), R[6]);
  ray.d1 = __fadd_rn(__fadd_rn(__fmul_rn(R[1], dcx), __fmul_rn(R[4], dcy)), R[7]);
  ray.d2 = __fadd_rn(__fadd_rn(__fmul_rn(R[2], dcx), __fmul_rn(R[5], dcy)), R[8]);
  const float dz = __fdiv_rn(step, sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dcx, dcx), __fmul_rn(dcy, dcy)), 1.0f)));

  // ---- which samples to look at (any arithmetic will do here, as long as it errs towards looking at more) -------------------------
  // In grid units the ray is g_a(n) = A_a + n D_a.  E bounds what the definition's fp32 g may differ from that by: a handful of
  // roundings of the largest magnitude involved, taken 16-fold, plus a floor.
  const float inv_voxel = 1.0f / v.voxel;
  const float A[3] = {(ray.e0 - v.o0) * inv_voxel, (ray.e1 - v.o1) * inv_voxel, (ray.e2 - v.o2) * inv_voxel};
  const float D[3] = {dz * ray.d0 * inv_voxel, dz * ray.d1 * inv_voxel, dz * ray.d2 * inv_voxel};
  const float hi[3] = {(float)(v.Nx - 1), (float)(v.Ny - 1), (float)(v.Nz - 1)};
  const float mag = fmaxf(fmaxf(fabsf(ray.e0) + fabsf(zfar * ray.d0) + fabsf(v.o0), fabsf(ray.e1) + fabsf(zfar * ray.d1) + fabsf(v.o1)),
                          fabsf(ray.e2) + fabsf(zfar * ray.d2) + fabsf(v.o2));
  const float E = 1e-6f * mag * inv_voxel + 1e-5f;
  float invD[3];
  float n_in = 1.0f, n_out = (float)n_max;
  bool meets = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    invD[a] = 1.0f / D[a];                                               // +-inf for a ray parallel to the axis
    if (fabsf(D[a]) > 1e-30f) {
      const float ta = (-2.0f * E - A[a]) * invD[a], tb = (hi[a] + 2.0f * E - A[a]) * invD[a];
      n_in = fmaxf(n_in, fminf(ta, tb));
      n_out = fminf(n_out, fmaxf(ta, tb));
    } else {
      meets = meets && A[a] >= -2.0f * E && A[a] <= hi[a] + 2.0f * E;
    }
  }
  // the slab test's own rounding: a relative 1e-5 and two samples on either side
  const float past = (float)(n_max + 1);
  int n = (int)fminf(past, fmaxf(1.0f, floorf(n_in * (1.0f - 1e-5f)) - 2.0f));
  const int n_last = (int)fminf((float)n_max, fmaxf(0.0f, ceilf(n_out * (1.0f + 1e-5f)) + 2.0f));
  if (znear > 0.0f) n = max(n, (int)fminf(past, fmaxf(1.0f, floorf(znear / dz * (1.0f - 1e-5f)) - 2.0f)));
  if (!meets || !(n_in <= n_out + 4.0f)) n = n_last + 1;                 // the ray passes the box by (or a NaN: no sample is inside)

  // ---- the march ------------------------------------------------------------------------------------------------------------------
  int n_hit = 0;
  float f_n = 0.0f;
  while (n <= n_last) {
    const float z = __fmul_rn((float)n, dz);
    if (!(z <= zfar)) break;
    if (v.bricks) {
      const CastCell cl = cell_at(v, ray, z);
      const int bx = cl.i >> 3, by = cl.j >> 3, bz = cl.k >> 3;
      const int nbx = (v.Nx + kBrick - 2) / kBrick, nby = (v.Ny + kBrick - 2) / kBrick;
      if (v.bricks[((size_t)bz * nby + by) * nbx + bx] == 0) {
        // samples n + 1 .. n + floor(k) stay within the brick's cells by more than 2 E: none of them can end the march
        const float g[3] = {cl.g0, cl.g1, cl.g2};
        const int b[3] = {bx, by, bz};
        float k = (float)(n_last - n);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float edge = D[a] > 0.0f ? (float)(b[a] * kBrick + kBrick) - 2.0f * E : (float)(b[a] * kBrick) + 2.0f * E;
          k = fminf(k, (edge - g[a]) * invD[a]);                         // a NaN (0 x inf) leaves k as it is
        }
        const int skip = (int)fmaxf(0.0f, floorf(k * (1.0f - 1e-4f)) - 1.0f);
        n += 1 + skip;
        continue;
      }
    }
    float f;
    if (sample_at(v, ray, z, znear, &f) && f < 0.0f) {
      n_hit = n;
      f_n = f;
      break;
    }
    ++n;
  }

  // ---- the first observed negative sample ended the march: a hit iff sample n - 1 (evaluated afresh) was observed too --------------
  float zd = 0.0f, nrm[3] = {0.0f, 0.0f, 0.0f}, col[3] = {0.0f, 0.0f, 0.0f}, wgt = 0.0f;
  float f_p = 0.0f;
  if (n_hit > 1 && sample_at(v, ray, __fmul_rn((float)(n_hit - 1), dz), znear, &f_p)) {
    zd = __fadd_rn(__fmul_rn((float)(n_hit - 1), dz), __fmul_rn(dz, __fdiv_rn(f_p, __fsub_rn(f_p, f_n))));
    const CastCell cl = cell_at(v, ray, zd);
    float f[8];
    if (out.normal) {
      gather8(v.tsdf, v, cl, f);
      const float gx = bilinear_ab(__fsub_rn(f[1], f[0]), __fsub_rn(f[3], f[2]), __fsub_rn(f[5], f[4]), __fsub_rn(f[7], f[6]), cl.m1, cl.m2);
      const float gy = bilinear_ab(__fsub_rn(f[2], f[0]), __fsub_rn(f[3], f[1]), __fsub_rn(f[6], f[4]), __fsub_rn(f[7], f[5]), cl.m0, cl.m2);
      const float gz = bilinear_ab(__fsub_rn(f[4], f[0]), __fsub_rn(f[5], f[1]), __fsub_rn(f[6], f[2]), __fsub_rn(f[7], f[3]), cl.m0, cl.m1);
      const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), __fmul_rn(gz, gz)));
      if (len > 0.0f) {                                                  // false for a NaN
        const float w0 = __fdiv_rn(gx, len), w1 = __fdiv_rn(gy, len), w2 = __fdiv_rn(gz, len);
#pragma unroll
        for (int a = 0; a < 3; ++a)
          nrm[a] = __fadd_rn(__fadd_rn(__fmul_rn(R[3 * a], w0), __fmul_rn(R[3 * a + 1], w1)), __fmul_rn(R[3 * a + 2], w2));
      }
    }
    if (out.rgb) {
      const size_t n_vox = (size_t)v.Nx * v.Ny * v.Nz;
      gather8(v.color4 + 3 * n_vox, v, cl, f);
      const float den = trilinear_ab(f, cl.m0, cl.m1, cl.m2);
      if (den > 0.0f) {
        for (int ch = 0; ch < 3; ++ch) {
          gather8(v.color4 + ch * n_vox, v, cl, f);
          col[ch] = __fdiv_rn(trilinear_ab(f, cl.m0, cl.m1, cl.m2), den);
        }
      }
    }
    if (out.weight) {
      gather8(v.wsum, v, cl, f);
      wgt = trilinear_ab(f, cl.m0, cl.m1, cl.m2);
    }
  }
  const size_t HW = (size_t)H * W, pix = (size_t)r * W + c;
  out.zdepth[(size_t)view * HW + pix] = zd;
  if (out.weight) out.weight[(size_t)view * HW + pix] = wgt;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (out.normal) out.normal[((size_t)view * 3 + a) * HW + pix] = nrm[a];
    if (out.rgb) out.rgb[((size_t)view * 3 + a) * HW + pix] = col[a];
  }
}

// One wavefront per brick, four bricks a workgroup; lane l looks at the 8 cells (x = l & 7, y = l >> 3, z = 0 .. 7) of its brick.
__global__ __launch_bounds__(256) void k_tsdf_bricks(const float* __restrict__ tsdf, const float* __restrict__ wsum, int Nx, int Ny, int Nz,
                                                     float min_weight, int nbx, int nby, long long n_bricks,
                                                     unsigned char* __restrict__ bricks) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long brick = blockIdx.x * 4LL + (threadIdx.x >> 6);         // the same for the whole wavefront
  if (brick >= n_bricks) return;
  const int bx = (int)(brick % nbx), by = (int)((brick / nbx) % nby), bz = (int)(brick / ((long long)nbx * nby));
  const int i = bx * kBrick + (lane & 7), j = by * kBrick + (lane >> 3);
  bool live = false;
  if (i < Nx - 1 && j < Ny - 1) {
    for (int z = 0; z < kBrick; ++z) {
      const int k = bz * kBrick + z;
      if (k >= Nz - 1) break;
      bool seen = true, neg = false;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const size_t at = ((size_t)(k + (q >> 2)) * Ny + (j + ((q >> 1) & 1))) * Nx + (i + (q & 1));
        seen = seen && wsum[at] > min_weight;
        neg = neg || tsdf[at] < 0.0f;
      }
      live = live || (seen && neg);
    }
  }
  const unsigned long long any = __ballot(live);
  if (lane == 0) bricks[brick] = any != 0ULL ? 1 : 0;
}

bool cast_dims_ok(int Nx, int Ny, int Nz) {
  return Nx >= 2 && Ny >= 2 && Nz >= 2 && Nx <= kCastMaxDim && Ny <= kCastMaxDim && Nz <= kCastMaxDim &&
         (long long)Nx * Ny * Nz <= 0x7fffffffLL;
}
int brick_dim(int N) { return (N - 1 + kBrick - 1) / kBrick; }

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" size_t diner_tsdf_bricks_bytes(int Nx, int Ny, int Nz) {
  if (!cast_dims_ok(Nx, Ny, Nz)) return 0;
  return (size_t)brick_dim(Nx) * brick_dim(Ny) * brick_dim(Nz);
}

extern "C" int diner_tsdf_bricks(const float* tsdf, const float* wsum, int Nx, int Ny, int Nz, float min_weight, unsigned char* bricks_out,
                                 void* stream) {
  DINER_CHECK_ARG(cast_dims_ok(Nx, Ny, Nz), "tsdf_bricks: volume dimension %d x %d x %d (each 2 .. %d, fewer than 2^31 samples)", Nx, Ny, Nz,
                  kCastMaxDim);
  DINER_CHECK_ARG(tsdf && wsum && bricks_out, "tsdf_bricks: null pointer argument");
  DINER_CHECK_ARG(min_weight == min_weight, "tsdf_bricks: min_weight is NaN");
  const int nbx = brick_dim(Nx), nby = brick_dim(Ny);
  const long long n_bricks = (long long)nbx * nby * brick_dim(Nz);
  hipLaunchKernelGGL(k_tsdf_bricks, dim3((unsigned)((n_bricks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, tsdf, wsum, Nx, Ny, Nz,
                     min_weight, nbx, nby, n_bricks, bricks_out);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_tsdf_raycast_f32(const float* tsdf, const float* wsum, const float* color4, int Nx, int Ny, int Nz, const float* origin,
                                      float voxel, const unsigned char* bricks, const float* intrinsics, const float* extrinsics, int V,
                                      int H, int W, float znear, float zfar, float step, float min_weight, float* zdepth_out,
                                      float* normal_out, float* rgb_out, float* weight_out, void* stream) {
  DINER_CHECK_ARG(V >= 1 && V <= kMaxViewsWide, "tsdf_raycast: %d views outside [1, %d]", V, kMaxViewsWide);
  DINER_CHECK_ARG(cast_dims_ok(Nx, Ny, Nz), "tsdf_raycast: volume dimension %d x %d x %d (each 2 .. %d, fewer than 2^31 samples)", Nx, Ny, Nz,
                  kCastMaxDim);
  DINER_CHECK_ARG(voxel > 0.0f && std::isfinite(voxel), "tsdf_raycast: voxel size %g (need > 0)", (double)voxel);
  DINER_CHECK_ARG(step > 0.0f && std::isfinite(step), "tsdf_raycast: step %g (need > 0 and finite)", (double)step);
  DINER_CHECK_ARG(znear >= 0.0f, "tsdf_raycast: znear %g (need >= 0)", (double)znear);
  DINER_CHECK_ARG(std::isfinite(zfar) && zfar > znear, "tsdf_raycast: zfar %g (need finite and > znear %g)", (double)zfar, (double)znear);
  DINER_CHECK_ARG(rgb_out == nullptr || color4 != nullptr, "tsdf_raycast: rgb_out without the color4 planes");
  DINER_CHECK_ARG(tsdf && wsum && origin && intrinsics && extrinsics && zdepth_out, "tsdf_raycast: null pointer argument");
  DINER_CHECK_ARG(min_weight == min_weight, "tsdf_raycast: min_weight is NaN");
  DINER_CHECK_ARG(H >= 1 && W >= 1 && (long long)V * 3 * H * W <= 0x7fffffffLL, "tsdf_raycast: bad map size %d x %d x %d", V, H, W);
  CastCams cams;
  memset(&cams, 0, sizeof(cams));
  // the trip count: the lattice index of zfar on the steepest ray -- |d_c| is convex in the pixel, so a corner pixel of some view
  double most = 0.0;
  bool finite = true;
  for (int n = 0; n < V; ++n) {
    const float* E = extrinsics + 16 * n;
    const float* Kn = intrinsics + 9 * n;
    CastCam& c = cams.cam[n];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) c.R[3 * a + b] = E[4 * a + b];
      c.t[a] = E[4 * a + 3];
    }
    c.fx = Kn[0];
    c.fy = Kn[4];
    c.cx = Kn[2];
    c.cy = Kn[5];
    for (int corner = 0; corner < 4; ++corner) {
      const double x = (((corner & 1) ? W - 1 : 0) + 0.5 - (double)c.cx) / (double)c.fx;
      const double y = (((corner & 2) ? H - 1 : 0) + 0.5 - (double)c.cy) / (double)c.fy;
      const double samples = (double)zfar * std::sqrt(x * x + y * y + 1.0) / (double)step;
      finite = finite && std::isfinite(samples);
      if (samples > most) most = samples;
    }
  }
  DINER_CHECK_ARG(finite, "tsdf_raycast: the cameras give no finite number of lattice samples on a ray");
  DINER_CHECK_ARG(most <= (double)kCastMaxSamples, "tsdf_raycast: %g lattice samples on a ray (at most %lld; step %g, zfar %g)", most,
                  kCastMaxSamples, (double)step, (double)zfar);
  const int n_max = (int)most + 2;
  const CastVolume vol = {tsdf, wsum, color4, bricks, Nx, Ny, Nz, origin[0], origin[1], origin[2], voxel, min_weight};
  const CastOut out = {zdepth_out, normal_out, rgb_out, weight_out};
  hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)((W + kCastTile - 1) / kCastTile), (unsigned)((H + kCastTile - 1) / kCastTile), (unsigned)V),
                     dim3(256), 0, (hipStream_t)stream, vol, cams, H, W, znear, zfar, step, n_max, out);
  DINER_LAUNCH_OK();
  return 0;
}
