// The training objective on the device: what DINER.calc_losses does around renderer.forward (reference src/models/diner.py:217-290)
//   k_sample_patch   the s x s ray patch of the step, its centre drawn from the target's foreground mask      (diner.py:233-247)
//   k_objective      MSELoss + w_antibias * AntibiasLoss on the rendered patch, value and gradient in one pass (diner.py:265-288,
//                    src/losses/antibiasloss.py:4-14), with the gather of the ground-truth colours folded in
// (rays at the listed pixels: k_gen_rays_at, prep.hip.)
//
// Arithmetic: p - g rounds to float32 as the reference's subtraction does; every sum is double.  No floating-point atomics: each
// workgroup writes its partial sums to its own workspace slot and k_objective_finalize adds the slots in a fixed order (the scheme
// of metrics.hip), so the three losses and d_pred are bit-identical from run to run and between the two ground-truth routes.
#include "common.hpp"

namespace diner {

namespace {

constexpr int kObjThreads = 256;
constexpr int kObjMaxSide = 1024;                // patch side: 3 s signs of one row of cells in LDS
constexpr int kObjChunk = 3 * kObjThreads;       // values per workgroup without a patch (random-pixel mode)
constexpr int kPatchThreads = 1024;
constexpr uint32_t kPatchStream = 3u;            // Philox stream of the patch centre (0..2: the sampler's noise fields)

// ---- the patch of the step -----------------------------------------------------------------------------------------------------
// One workgroup per object.  Thread t owns the contiguous pixels [t chunk, (t + 1) chunk) of the row-major image; the weight of a pixel
// in the first / last `pad` rows and columns counts as 0, as does a weight that is not > 0.  Pass 1: the thread's sum (double, in pixel
// order); thread 0 turns the per-thread sums into exclusive prefixes in thread order.  Pass 2: every thread walks its pixels again from its
// prefix and reports the first one whose inclusive prefix exceeds u * total; the smallest such index (an integer minimum) is the centre.
__global__ void __launch_bounds__(kPatchThreads) k_sample_patch(const float* __restrict__ fg, int H, int W, int s, const float* __restrict__ u_in,
                                                                uint64_t seed, uint32_t step, int* __restrict__ pix, int* __restrict__ centres,
                                                                int* __restrict__ flags) {
  __shared__ double part[kPatchThreads];
  __shared__ double total_s;
  __shared__ int found;
  const int o = blockIdx.x, t = threadIdx.x;
  const int HW = H * W, pad = (s + 1) / 2;
  const float* w = fg + (size_t)o * HW;
  const int chunk = (HW + kPatchThreads - 1) / kPatchThreads;
  const int p0 = min(t * chunk, HW), p1 = min(p0 + chunk, HW);
  auto weight = [&](int p) -> double {
    const int y = p / W, x = p - y * W;
    const float v = w[p];
    return (x >= pad && x < W - pad && y >= pad && y < H - pad && v > 0.0f) ? (double)v : 0.0;
  };
  double acc = 0.0;
  for (int p = p0; p < p1; ++p) acc += weight(p);
  part[t] = acc;
  if (t == 0) found = HW;
  __syncthreads();
  if (t == 0) {
    double run = 0.0;
    for (int k = 0; k < kPatchThreads; ++k) {
      const double v = part[k];
      part[k] = run;
      run += v;
    }
    total_s = run;
  }
  __syncthreads();
  const double total = total_s;
  float u = u_in ? u_in[o] : rng_uniform(seed, kPatchStream, step, (uint32_t)o);
  u = fminf(fmaxf(u, 0.0f), 0.99999994f);        // [0, 1); NaN -> 0
  const double target = (double)u * total;
  if (total > 0.0) {
    double run = part[t];
    for (int p = p0; p < p1; ++p) {
      run += weight(p);
      if (run > target) {
        atomicMin(&found, p);
        break;
      }
    }
  }
  __syncthreads();
  const int c = found;
  const bool ok = total > 0.0 && c < HW;
  const int cy = ok ? c / W : H / 2, cx = ok ? c - (c / W) * W : W / 2;
  if (t == 0) {
    centres[2 * o] = cx;
    centres[2 * o + 1] = cy;
    flags[o] = ok ? 0 : 1;
  }
  for (int k = t; k < s * s; k += kPatchThreads) {
    const int i = k / s, j = k - i * s;
    const int y = min(max(cy - pad + i, 0), H - 1), x = min(max(cx - pad + j, 0), W - 1);      // inside the image for every centre above
    pix[(size_t)o * s * s + k] = y * W + x;
  }
}

// ---- MSE + anti-bias -------------------------------------------------------------------------------------------------------------
struct ObjArgs {
  const float* pred;       // (SB, B, 3)
  const float* gt;         // (SB, B, 3) or NULL
  const float* images;     // (SB, 3, H, W) with pix (SB, B) when gt is NULL
  const int* pix;
  int B, HW, s, c, n_bands;
  double g_mse, g_ab;      // w_mse * 2 / (SB B 3);  w_antibias / (c^2 SB 3 (s / c)^2)
  double inv_cell;         // 1 / c^2
};

__device__ __forceinline__ float obj_diff(const ObjArgs& a, int o, int pixel, int ch) {
  const float p = a.pred[((size_t)o * a.B + pixel) * 3 + ch];
  float g;
  if (a.gt) {
    g = a.gt[((size_t)o * a.B + pixel) * 3 + ch];
  } else {
    const int q = min(max(a.pix[(size_t)o * a.B + pixel], 0), a.HW - 1);
    g = a.images[((size_t)o * 3 + ch) * a.HW + q];
  }
  return __fsub_rn(p, g);
}

// One workgroup per (object, band).  With a patch a band is one row of cells (c rows x s columns x 3 channels of the patch, contiguous in
// pred); without one it is a chunk of kObjChunk values.  Groups of L = min(64, c^2) lanes sum the differences of one cell of one channel
// (lane l takes pixels l, l + L, ... of the cell, then a fixed xor tree), the sign of the cell goes to LDS, and a second pass over the
// band's values writes d_pred.  ws slot of the workgroup: {sum d^2, sum |D|}.
__global__ void __launch_bounds__(kObjThreads) k_objective(ObjArgs a, double* __restrict__ ws, float* __restrict__ d_pred) {
  __shared__ float sgn[3 * kObjMaxSide];
  __shared__ double red[kObjThreads / 64];
  const int t = threadIdx.x, o = blockIdx.y, band = blockIdx.x;
  const int s = a.s, c = a.c;
  const int v0 = s > 0 ? band * c * s * 3 : band * kObjChunk;                  // first value of the band within the object
  const int nv = s > 0 ? c * s * 3 : min(kObjChunk, a.B * 3 - v0);
  double ab = 0.0;
  if (s > 0) {
    const int cells = s / c, ncc = cells * 3, cc2 = c * c;
    const int L = cc2 < 64 ? cc2 : 64;
    const int n_items = ncc * L;
    for (int it0 = 0; it0 < n_items; it0 += kObjThreads) {                      // uniform: every lane reaches the shuffles
      const int it = it0 + t;
      const bool on = it < n_items;
      const int cc = on ? it / L : 0, l = it - (it / L) * L;
      const int cell = cc / 3, ch = cc - cell * 3;
      double sum = 0.0;
      if (on)
        for (int q = l; q < cc2; q += L) {
          const int r = q / c, x = cell * c + (q - r * c);
          sum += (double)obj_diff(a, o, (band * c + r) * s + x, ch);
        }
      for (int off = L >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
      if (on && l == 0) {
        const double D = sum * a.inv_cell;
        sgn[cc] = D > 0.0 ? 1.0f : (D < 0.0 ? -1.0f : 0.0f);                   // sign(0) = 0 (and NaN -> 0), as L1Loss's backward
        ab += fabs(D);
      }
    }
    __syncthreads();
  }
  double mse = 0.0;
  for (int v = t; v < nv; v += kObjThreads) {
    const int gv = v0 + v;
    const int pixel = gv / 3, ch = gv - pixel * 3;
    const float d = obj_diff(a, o, pixel, ch);
    mse += (double)d * (double)d;
    double g = a.g_mse * (double)d;
    if (s > 0) {
      const int x = pixel - (pixel / s) * s;
      g += a.g_ab * (double)sgn[(x / c) * 3 + ch];
    }
    d_pred[(size_t)o * a.B * 3 + gv] = (float)g;
  }
  mse = block_sum_d<kObjThreads / 64>(mse, red);
  ab = block_sum_d<kObjThreads / 64>(ab, red);
  if (t == 0) {
    double* slot = ws + ((size_t)o * a.n_bands + band) * 2;
    slot[0] = mse;
    slot[1] = ab;
  }
}

// One wave: lane l adds slots l, l + 64, ..., then a fixed xor tree.  -> losses = {rgb_fine, antibias, w_mse rgb_fine + w_antibias antibias}
__global__ void __launch_bounds__(64) k_objective_finalize(const double* __restrict__ ws, int n_slots, double n_mse, double n_ab, double w_mse,
                                                           double w_ab, double* __restrict__ losses) {
  double m = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < n_slots; k += 64) {
    m += ws[(size_t)k * 2];
    b += ws[(size_t)k * 2 + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m += __shfl_xor(m, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if (threadIdx.x == 0) {
    const double l_mse = m / n_mse, l_ab = n_ab > 0.0 ? b / n_ab : 0.0;
    losses[0] = l_mse;
    losses[1] = l_ab;
    losses[2] = w_mse * l_mse + w_ab * l_ab;
  }
}

// 0 when the sizes are ones the objective takes; *n_bands = workgroups per object
int objective_plan(int SB, int B, int s, int n_down, int* n_bands, const char* who) {
  DINER_CHECK_ARG(SB >= 1 && SB <= 65535, "%s: SB = %d objects, need 1 <= SB <= 65535", who, SB);
  DINER_CHECK_ARG(B >= 1 && B <= (1 << 24), "%s: B = %d rays per object, need 1 <= B <= 2^24", who, B);
  DINER_CHECK_ARG(s >= 0 && s <= kObjMaxSide, "%s: patch side s = %d, need 0 <= s <= %d", who, s, kObjMaxSide);
  if (s == 0) {
    *n_bands = (B * 3 + kObjChunk - 1) / kObjChunk;
    return 0;
  }
  DINER_CHECK_ARG(n_down >= 0 && n_down <= 10, "%s: n_downsampling = %d, need 0 <= n <= 10", who, n_down);
  DINER_CHECK_ARG((long long)s * s == B, "%s: B = %d rays is not the s x s = %d x %d patch", who, B, s, s);
  DINER_CHECK_ARG(s % (1 << n_down) == 0, "%s: patch side s = %d is not a multiple of 2^n = %d", who, s, 1 << n_down);
  *n_bands = s >> n_down;
  return 0;
}

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" int diner_sample_patch(const float* fg, int SB, int H, int W, int s, const float* u, uint64_t seed, long long step, int* pix_idcs,
                                  int* centres, int* flags, void* stream) {
  DINER_CHECK_ARG(fg && pix_idcs && centres && flags, "sample_patch: null pointer argument");
  DINER_CHECK_ARG(SB >= 1 && SB <= 65535, "sample_patch: SB = %d objects, need 1 <= SB <= 65535", SB);
  DINER_CHECK_ARG(H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "sample_patch: bad image size %d x %d", W, H);
  DINER_CHECK_ARG(s >= 1, "sample_patch: patch side s = %d, need s >= 1", s);
  DINER_CHECK_ARG(s + 1 <= (H < W ? H : W), "sample_patch: patch side s = %d: s + 1 exceeds min(H, W) = %d", s, H < W ? H : W);
  hipLaunchKernelGGL(k_sample_patch, dim3(SB), dim3(kPatchThreads), 0, (hipStream_t)stream, fg, H, W, s, u, seed, (uint32_t)step, pix_idcs,
                     centres, flags);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" size_t diner_objective_workspace_bytes(int SB, int B, int s, int n_downsampling) {
  int n_bands = 0;
  if (objective_plan(SB, B, s, n_downsampling, &n_bands, "objective_workspace_bytes") != 0) return 0;
  return (size_t)SB * n_bands * 2 * sizeof(double);
}

extern "C" int diner_objective_f32(const float* pred, const float* gt, const float* images, const int* pix, int SB, int B, int H, int W, int s,
                                   int n_downsampling, double w_mse, double w_antibias, void* workspace, double* losses, float* d_pred,
                                   void* stream) {
  DINER_CHECK_ARG(pred && workspace && losses && d_pred, "objective: null pointer argument");
  DINER_CHECK_ARG(gt || (images && pix), "objective: null pointer argument (the ground truth is gt, or images with pix)");
  int n_bands = 0;
  const int rc = objective_plan(SB, B, s, n_downsampling, &n_bands, "objective");
  if (rc) return rc;
  DINER_CHECK_ARG(w_mse >= 0.0 && w_antibias >= 0.0, "objective: weights w_mse = %g, w_antibias = %g must be >= 0", w_mse, w_antibias);
  DINER_CHECK_ARG(s > 0 || w_antibias == 0.0, "objective: the anti-bias term needs a patch (B = %d rays, s = 0): B != s * s", B);
  if (!gt) DINER_CHECK_ARG(H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "objective: bad image size %d x %d", W, H);
  ObjArgs a;
  a.pred = pred;
  a.gt = gt;
  a.images = gt ? nullptr : images;
  a.pix = gt ? nullptr : pix;
  a.B = B;
  a.HW = gt ? 1 : H * W;
  a.s = s;
  a.c = s > 0 ? 1 << n_downsampling : 1;
  a.n_bands = n_bands;
  const double n_mse = (double)SB * B * 3;
  const double n_cells = s > 0 ? (double)SB * 3 * (s / a.c) * (s / a.c) : 0.0;
  a.inv_cell = 1.0 / ((double)a.c * a.c);
  a.g_mse = w_mse * 2.0 / n_mse;
  a.g_ab = s > 0 ? w_antibias / ((double)a.c * a.c * n_cells) : 0.0;
  hipLaunchKernelGGL(k_objective, dim3(n_bands, SB), dim3(kObjThreads), 0, (hipStream_t)stream, a, (double*)workspace, d_pred);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_objective_finalize, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, SB * n_bands, n_mse, n_cells,
                     w_mse, w_antibias, losses);
  DINER_LAUNCH_OK();
  return 0;
}
