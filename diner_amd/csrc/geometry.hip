// Geometry from a render: what turns the compositor's per-sample weights into a surface, and the multi-view clean-up of the result.
//
// diner_ray_geometry_f32: one reduction over the weights (NR,K) the compositor writes on request, the z (NR,K) and the rays (NR,8) it was
// given.  One wavefront per ray in the compositor's layout (lane l holds per_lane consecutive samples: 4 per lane up to K = 256, 16 up
// to 1024).  With w_k the weights in sample order:
//   c_k        = sum_{j<=k} w_j: the lane's running sum in sample order + the sum of the lanes before it (an inclusive additive wave
//                scan of the lane totals, shifted by one lane);
//   A          = c_{K-1}, the last element of that same sequence (NOT a separately reduced sum), so that c_{K-1} >= quantile * A holds
//                whatever the rounding and an index always exists;
//   valid      iff A > alpha_min (a NaN A is invalid); an invalid ray writes 0 to every float output and -1 to median_idx;
//   median_idx = min{k : c_k >= quantile * A} -- "first k" keeps it defined where a weight is negative (a sample beyond `far`);
//   depth_median = z[median_idx];  depth_mean = (sum_k w_k z_k) / A;  t = depth_median (point_mode 0) or depth_mean (point_mode 1);
//   points = o + t d;  zdepth = t (d . cam_fwd), cam_fwd = row 2 of the target's world->camera rotation: the camera-z depth that
//   depth2normal (prep.hip, point_at) and the encoder take, where the compositor's depth is a distance along the normalised ray.
//
// diner_depth_consistency_f32: the cross-view check of N z-depth maps, one thread per (reference view r, pixel) with a loop over the
// other views s -- check_geometric_consistency / reproject_with_depth and the averaging of filter_depth of the reference's
// deps/TransMVSNet/dynamic_fusion.py with one threshold pair, THIS project's pixel centres at +0.5 (prep.hip) and a stricter bilinear
// tap rule (all four taps inside the image and non-zero, where cv2.remap blends with zeros).
#include "common.hpp"

namespace diner {

namespace {

constexpr int kGeoShortPerLane = 4;      // K <= 256, as kCompMaxPerLane of composite.hip
constexpr int kGeoLongPerLane = 16;      // K <= 1024, as kCompLongPerLane
constexpr int kGeoNoIndex = 0x7fffffff;

struct RayGeoOut {
  float* depth_median;
  int* median_idx;
  float* depth_mean;
  float* zdepth;
  float* points;
};

template <int kPerLane>
__global__ __launch_bounds__(256) void k_ray_geometry(const float* __restrict__ weights, const float* __restrict__ z,
                                                      const float* __restrict__ rays, int NR, int K, int per_lane, float quantile,
                                                      float alpha_min, float fwd0, float fwd1, float fwd2, int point_mode,
                                                      RayGeoOut out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + wave;
  if (ray >= NR) return;                      // no block-level sync below: waves are independent
  const float* wr = weights + (size_t)ray * K;
  const float* zr = z + (size_t)ray * K;

  float c[kPerLane];                          // the lane's running sums in sample order
  float run = 0.0f, wz = 0.0f;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int k = lane * per_lane + j;
    if (j < per_lane && k < K) {
      const float w = wr[k];
      run += w;
      wz += w * zr[k];
    }
    c[j] = run;
  }
  float incl = run;                           // inclusive additive scan of the lane totals
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const float up = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += up;
  }
  float before = __shfl_up(incl, 1, kWave);   // the lanes before this one
  if (lane == 0) before = 0.0f;
  const int last_lane = (K - 1) / per_lane;   // holds sample K-1; per_lane = ceil(K / 64) keeps it below 64
  const float A = __shfl(before + run, last_lane, kWave);       // c_{K-1}
  const float thr = __fmul_rn(quantile, A);
  int first = kGeoNoIndex;
#pragma unroll
  for (int j = kPerLane - 1; j >= 0; --j) {
    const int k = lane * per_lane + j;
    if (j < per_lane && k < K && before + c[j] >= thr) first = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, kWave));
  wz = wave_sum(wz);
  if (lane != 0) return;

  const bool valid = A > alpha_min;           // false for a NaN
  // valid: A > 0 and quantile <= 1 give thr <= A = c_{K-1}, so `first` is an index; the clamp is there for the bounds of the read only
  const int idx = valid ? min(first, K - 1) : -1;
  float d_med = 0.0f, d_mean = 0.0f, t = 0.0f;
  if (valid) {
    d_med = zr[idx];
    d_mean = __fdiv_rn(wz, A);
    t = point_mode == 0 ? d_med : d_mean;
  }
  if (out.depth_median) out.depth_median[ray] = d_med;
  if (out.median_idx) out.median_idx[ray] = idx;
  if (out.depth_mean) out.depth_mean[ray] = d_mean;
  if (out.zdepth || out.points) {
    const float* r = rays + (size_t)ray * 8;
    const float d0 = r[3], d1 = r[4], d2 = r[5];
    if (out.zdepth) {
      const float cosine = __fadd_rn(__fadd_rn(__fmul_rn(d0, fwd0), __fmul_rn(d1, fwd1)), __fmul_rn(d2, fwd2));
      out.zdepth[ray] = valid ? __fmul_rn(t, cosine) : 0.0f;
    }
    if (out.points) {
      float* p = out.points + (size_t)ray * 3;
      p[0] = valid ? __fadd_rn(r[0], __fmul_rn(t, d0)) : 0.0f;
      p[1] = valid ? __fadd_rn(r[1], __fmul_rn(t, d1)) : 0.0f;
      p[2] = valid ? __fadd_rn(r[2], __fmul_rn(t, d2)) : 0.0f;
    }
  }
}

// Kernel-argument cameras of the consistency check: 16 floats per view, 1 KiB for DINER_MAX_VIEWS, like RayCams of prep.hip.
struct GeoCam {        // R (world->cam, row-major), t, fx, fy, cx, cy
  float R[9], t[3], fx, fy, cx, cy;
};
struct GeoCams {
  GeoCam cam[kMaxViewsWide];
};

// camera-frame point of pixel coordinates (u, v) at z-depth d: ((u - cx) / fx d, (v - cy) / fy d, d)
__device__ __forceinline__ void back_project(const GeoCam& c, float u, float v, float d, float& x, float& y, float& zc) {
  x = __fmul_rn(__fdiv_rn(__fsub_rn(u, c.cx), c.fx), d);
  y = __fmul_rn(__fdiv_rn(__fsub_rn(v, c.cy), c.fy), d);
  zc = d;
}
// x_w = R^T (x_c - t)
__device__ __forceinline__ void cam_to_world(const GeoCam& c, float x, float y, float zc, float& w0, float& w1, float& w2) {
  const float a = __fsub_rn(x, c.t[0]), b = __fsub_rn(y, c.t[1]), e = __fsub_rn(zc, c.t[2]);
  w0 = __fadd_rn(__fadd_rn(__fmul_rn(c.R[0], a), __fmul_rn(c.R[3], b)), __fmul_rn(c.R[6], e));
  w1 = __fadd_rn(__fadd_rn(__fmul_rn(c.R[1], a), __fmul_rn(c.R[4], b)), __fmul_rn(c.R[7], e));
  w2 = __fadd_rn(__fadd_rn(__fmul_rn(c.R[2], a), __fmul_rn(c.R[5], b)), __fmul_rn(c.R[8], e));
}
// x_c = R x_w + t
__device__ __forceinline__ void world_to_geo_cam(const GeoCam& c, float w0, float w1, float w2, float& x, float& y, float& zc) {
  x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.R[0], w0), __fmul_rn(c.R[1], w1)), __fmul_rn(c.R[2], w2)), c.t[0]);
  y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.R[3], w0), __fmul_rn(c.R[4], w1)), __fmul_rn(c.R[5], w2)), c.t[1]);
  zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.R[6], w0), __fmul_rn(c.R[7], w1)), __fmul_rn(c.R[8], w2)), c.t[2]);
}
// pixel coordinates (centres at +0.5) of a camera-frame point: fx x / z + cx
__device__ __forceinline__ void project_px(const GeoCam& c, float x, float y, float zc, float& u, float& v) {
  u = __fadd_rn(__fmul_rn(c.fx, __fdiv_rn(x, zc)), c.cx);
  v = __fadd_rn(__fmul_rn(c.fy, __fdiv_rn(y, zc)), c.cy);
}

__global__ __launch_bounds__(256) void k_depth_consistency(const float* __restrict__ depth, GeoCams cams, int N, int H, int W,
                                                           float px_thr, float rel_thr, int* __restrict__ count_out,
                                                           float* __restrict__ depth_avg_out) {
  const long long HW = (long long)H * W;
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)N * HW) return;
  const int r = (int)(idx / HW);
  const int rem = (int)(idx - (long long)r * HW);
  const int i = rem / W, j = rem - i * W;
  const float D = depth[idx];
  int count = 0;
  float sum = D;
  if (D != 0.0f) {
    const GeoCam& cr = cams.cam[r];
    const float uc = (float)j + 0.5f, vc = (float)i + 0.5f;
    float x, y, zc, w0, w1, w2;
    back_project(cr, uc, vc, D, x, y, zc);
    cam_to_world(cr, x, y, zc, w0, w1, w2);
    for (int s = 0; s < N; ++s) {
      if (s == r) continue;
      const GeoCam& cs = cams.cam[s];
      float xs, ys, zs, u, v;
      world_to_geo_cam(cs, w0, w1, w2, xs, ys, zs);
      if (!(zs > 0.0f)) continue;                                   // behind s (or NaN)
      project_px(cs, xs, ys, zs, u, v);
      const float px = __fsub_rn(u, 0.5f), py = __fsub_rn(v, 0.5f);  // texel coordinates of the bilinear lookup
      if (!(px >= 0.0f && px < (float)(W - 1) && py >= 0.0f && py < (float)(H - 1))) continue;   // a tap outside (or NaN)
      const int x0 = (int)px, y0 = (int)py;                          // floor: both are >= 0; x0 + 1 <= W - 1, y0 + 1 <= H - 1
      const float ax = __fsub_rn(px, (float)x0), ay = __fsub_rn(py, (float)y0);
      const float* ds = depth + (size_t)s * HW + (size_t)y0 * W + x0;
      const float d00 = ds[0], d01 = ds[1], d10 = ds[W], d11 = ds[W + 1];
      if (d00 == 0.0f || d01 == 0.0f || d10 == 0.0f || d11 == 0.0f) continue;     // a tap without a surface
      const float bx = __fsub_rn(1.0f, ax), by = __fsub_rn(1.0f, ay);
      const float Ds = __fadd_rn(__fadd_rn(__fmul_rn(__fmul_rn(bx, by), d00), __fmul_rn(__fmul_rn(ax, by), d01)),
                                 __fadd_rn(__fmul_rn(__fmul_rn(bx, ay), d10), __fmul_rn(__fmul_rn(ax, ay), d11)));
      float v0, v1, v2, xr, yr, dr, u2, v2p;
      back_project(cs, u, v, Ds, xs, ys, zs);
      cam_to_world(cs, xs, ys, zs, v0, v1, v2);
      world_to_geo_cam(cr, v0, v1, v2, xr, yr, dr);
      project_px(cr, xr, yr, dr, u2, v2p);
      const float du = __fsub_rn(u2, uc), dv = __fsub_rn(v2p, vc);
      const float dist = __fsqrt_rn(__fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv)));
      const float rel = __fdiv_rn(fabsf(__fsub_rn(dr, D)), D);
      if (dist < px_thr && rel < rel_thr) {                          // a NaN is inconsistent
        ++count;
        sum = __fadd_rn(sum, dr);
      }
    }
  }
  if (count_out) count_out[idx] = count;
  if (depth_avg_out) depth_avg_out[idx] = D != 0.0f ? __fdiv_rn(sum, (float)(count + 1)) : 0.0f;
}

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" int diner_ray_geometry_f32(const float* weights, const float* z, const float* rays, int NR, int K, float quantile,
                                      float alpha_min, const float* cam_fwd, int point_mode, float* depth_median_out,
                                      int* median_idx_out, float* depth_mean_out, float* zdepth_out, float* points_out, void* stream) {
  DINER_CHECK_ARG(weights && z && rays, "ray_geometry: null pointer argument");
  DINER_CHECK_ARG(NR >= 1, "ray_geometry: NR = %d (need >= 1)", NR);
  DINER_CHECK_ARG(K >= 1 && K <= kWave * kGeoLongPerLane, "ray_geometry: K = %d outside [1, %d]", K, kWave * kGeoLongPerLane);
  DINER_CHECK_ARG(quantile > 0.0f && quantile <= 1.0f, "ray_geometry: quantile %g outside (0, 1]", (double)quantile);
  DINER_CHECK_ARG(alpha_min >= 0.0f, "ray_geometry: alpha_min %g (need >= 0)", (double)alpha_min);
  DINER_CHECK_ARG(point_mode == 0 || point_mode == 1, "ray_geometry: point_mode %d (0: median, 1: mean)", point_mode);
  DINER_CHECK_ARG(cam_fwd || !zdepth_out, "ray_geometry: zdepth needs cam_fwd, row 2 of the world->camera rotation");
  const int per_lane = (K + kWave - 1) / kWave;
  const float f0 = cam_fwd ? cam_fwd[0] : 0.0f, f1 = cam_fwd ? cam_fwd[1] : 0.0f, f2 = cam_fwd ? cam_fwd[2] : 0.0f;
  const RayGeoOut out = {depth_median_out, median_idx_out, depth_mean_out, zdepth_out, points_out};
  if (K <= kWave * kGeoShortPerLane)
    hipLaunchKernelGGL(k_ray_geometry<kGeoShortPerLane>, dim3((NR + 3) / 4), dim3(256), 0, (hipStream_t)stream, weights, z, rays, NR, K,
                       per_lane, quantile, alpha_min, f0, f1, f2, point_mode, out);
  else
    hipLaunchKernelGGL(k_ray_geometry<kGeoLongPerLane>, dim3((NR + 3) / 4), dim3(256), 0, (hipStream_t)stream, weights, z, rays, NR, K,
                       per_lane, quantile, alpha_min, f0, f1, f2, point_mode, out);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_depth_consistency_f32(const float* depth, const float* intrinsics, const float* extrinsics, int N, int H, int W,
                                           float px_thr, float rel_thr, int* count_out, float* depth_avg_out, void* stream) {
  DINER_CHECK_ARG(depth && intrinsics && extrinsics, "depth_consistency: null pointer argument");
  DINER_CHECK_ARG(N >= 2 && N <= kMaxViewsWide, "depth_consistency: %d views outside [2, %d]", N, kMaxViewsWide);
  DINER_CHECK_ARG(H >= 1 && W >= 1 && (long long)N * H * W <= 0x7fffffffLL, "depth_consistency: bad map size %d x %d x %d", N, H, W);
  DINER_CHECK_ARG(px_thr >= 0.0f && rel_thr >= 0.0f, "depth_consistency: thresholds %g, %g (need >= 0)", (double)px_thr, (double)rel_thr);
  GeoCams cams;
  memset(&cams, 0, sizeof(cams));
  for (int n = 0; n < N; ++n) {
    const float* E = extrinsics + 16 * n;
    const float* Kn = intrinsics + 9 * n;
    GeoCam& c = cams.cam[n];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) c.R[3 * a + b] = E[4 * a + b];
      c.t[a] = E[4 * a + 3];
    }
    c.fx = Kn[0];
    c.fy = Kn[4];
    c.cx = Kn[2];
    c.cy = Kn[5];
  }
  const long long total = (long long)N * H * W;
  hipLaunchKernelGGL(k_depth_consistency, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, cams, N, H, W,
                     px_thr, rel_thr, count_out, depth_avg_out);
  DINER_LAUNCH_OK();
  return 0;
}
