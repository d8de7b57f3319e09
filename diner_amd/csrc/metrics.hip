// Image-quality metrics on the device: what the reference's evaluate_folder computes per image pair (eval_suite.py:62-68) on 8-bit
// images -- l1 (mean |p - g|), l2 (skimage mean_squared_error), psnr (data_range 1) and ssim (skimage structural_similarity with its
// defaults: 7x7 uniform window, K1 0.01, K2 0.03, sample covariance, map cropped by 3 px, mean over the 3 channels).
//
// A pixel value is the float32 fl32(k) / 255 (`astype(np.float32) / 255.0`), read from a 256-entry table.  p - g and its square round
// to float32 as numpy does; the sums of |d| and d^2, the window moments and the per-pixel S are double.  No floating-point atomics:
// each workgroup writes its partial sums to its own workspace slot and k_metrics_finalize adds the slots of one image in a fixed
// order, so the scores are bit-identical across runs, across positions in a batch and between the two input routes (the fp32 route
// quantises to the same bytes in-kernel before anything else happens).
#include "common.hpp"

namespace diner {

namespace {

constexpr int kMetThreads = 256;                 // one thread per staged column
constexpr int kMetHalo = 3;                      // (7 - 1) / 2
constexpr int kMetTileW = kMetThreads - 2 * kMetHalo;   // 250 columns owned per workgroup
constexpr int kMetBand = 32;                     // rows owned per workgroup
constexpr int kMetRows = kMetBand + 2 * kMetHalo;
constexpr int kMetSlot = 3;                      // {sum |d|, sum d^2, sum S} per workgroup

struct U8Table {
  float v[256];
};
constexpr U8Table make_u8_table() {              // constant-folded, correctly rounded: fl32(k) / 255 in float32
  U8Table t{};
  for (int k = 0; k < 256; ++k) t.v[k] = (float)k / 255.0f;
  return t;
}
__constant__ U8Table kU8Table = make_u8_table();

// Input routes: byte at (image n, channel ch, row r, column c) of the pair.
struct SrcU8 {
  const unsigned char* pred;
  const unsigned char* gt;
  int pred_c, gt_c;
  __device__ __forceinline__ void load(int n, int ch, int H, int W, int r, int c, unsigned char& p, unsigned char& g) const {
    const size_t px = ((size_t)n * H + r) * W + c;
    p = pred[px * pred_c + ch];
    g = gt[px * gt_c + ch];
  }
};
struct SrcF32 {          // (N,3,H,W) planar, quantised as save_image / k_quantize_rgb do
  const float* pred;
  const float* gt;
  __device__ __forceinline__ void load(int n, int ch, int H, int W, int r, int c, unsigned char& p, unsigned char& g) const {
    const size_t i = (((size_t)n * 3 + ch) * H + r) * W + c;
    p = quantize_u8(pred[i]);
    g = quantize_u8(gt[i]);
  }
};

// One workgroup per (band of kMetBand rows, tile of kMetTileW columns, channel, image).  Thread t stages column c0 - 3 + t of the
// band's rows plus a 3-row / 3-column halo, forms the vertical 7-sums of the five moments at its column for each centre row, and the
// threads owning a column add the horizontal 7-sums into S.  L1 / L2 run over every owned pixel (they are not cropped).
template <class Src>
__global__ void __launch_bounds__(kMetThreads) k_metrics_partial(Src src, int H, int W, int n_tiles, double* __restrict__ ws) {
  __shared__ unsigned char sp[kMetRows][kMetThreads];
  __shared__ unsigned char sg[kMetRows][kMetThreads];
  __shared__ float tab[256];
  __shared__ double vs[5][kMetThreads];
  __shared__ double red[kMetThreads / 64];
  const int t = threadIdx.x;
  const int band = blockIdx.x / n_tiles, tile = blockIdx.x - band * n_tiles;
  const int ch = blockIdx.y, n = blockIdx.z;
  const int r0 = band * kMetBand;
  const int c = tile * kMetTileW - kMetHalo + t;
  const bool col_in = c >= 0 && c < W;
  tab[t] = kU8Table.v[t];
  for (int lr = 0; lr < kMetRows; ++lr) {
    const int r = r0 - kMetHalo + lr;
    unsigned char p = 0, g = 0;
    if (col_in && r >= 0 && r < H) src.load(n, ch, H, W, r, c, p, g);
    sp[lr][t] = p;
    sg[lr][t] = g;
  }
  __syncthreads();

  const bool owner = t >= kMetHalo && t < kMetThreads - kMetHalo && col_in;
  double l1 = 0.0, l2 = 0.0, ss = 0.0;
  if (owner) {
    const int r_end = min(r0 + kMetBand, H);
    for (int r = r0; r < r_end; ++r) {
      const int lr = r - r0 + kMetHalo;
      const float d = __fsub_rn(tab[sp[lr][t]], tab[sg[lr][t]]);
      l1 += (double)fabsf(d);
      l2 += (double)__fmul_rn(d, d);
    }
  }

  const double inv_np = 1.0 / 49.0;
  const double cov_norm = 49.0 / 48.0;
  const double C1 = (0.01 * 1.0) * (0.01 * 1.0), C2 = (0.03 * 1.0) * (0.03 * 1.0);
  const bool centre_col = owner && c >= kMetHalo && c < W - kMetHalo;
  const int i0 = max(r0, kMetHalo), i1 = min(r0 + kMetBand, H - kMetHalo);
  for (int i = i0; i < i1; ++i) {                // uniform across the workgroup: every thread reaches both barriers
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    if (col_in) {
      const int lr0 = i - r0;                    // staged row of i - 3
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const double x = (double)tab[sp[lr0 + k][t]], y = (double)tab[sg[lr0 + k][t]];
        sx += x;
        sy += y;
        sxx += x * x;
        syy += y * y;
        sxy += x * y;
      }
    }
    vs[0][t] = sx;
    vs[1][t] = sy;
    vs[2][t] = sxx;
    vs[3][t] = syy;
    vs[4][t] = sxy;
    __syncthreads();
    if (centre_col) {
      double m[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double s = 0.0;
#pragma unroll
        for (int k = -kMetHalo; k <= kMetHalo; ++k) s += vs[q][t + k];
        m[q] = s * inv_np;
      }
      const double ux = m[0], uy = m[1];
      const double vx = cov_norm * (m[2] - ux * ux);
      const double vy = cov_norm * (m[3] - uy * uy);
      const double vxy = cov_norm * (m[4] - ux * uy);
      const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
      const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
      ss += (A1 * A2) / (B1 * B2);
    }
    __syncthreads();
  }

  l1 = block_sum_d<kMetThreads / 64>(l1, red);
  l2 = block_sum_d<kMetThreads / 64>(l2, red);
  ss = block_sum_d<kMetThreads / 64>(ss, red);
  if (t == 0) {
    const int n_slots = gridDim.x;
    double* o = ws + (((size_t)n * 3 + ch) * n_slots + blockIdx.x) * kMetSlot;
    o[0] = l1;
    o[1] = l2;
    o[2] = ss;
  }
}

// One wave per image: lane l adds slots l, l + 64, ... of each channel, then a fixed xor tree.  -> out[n] = {l1, l2, psnr, ssim}
__global__ void __launch_bounds__(64) k_metrics_finalize(const double* __restrict__ ws, int n_slots, int H, int W,
                                                         double* __restrict__ out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  double l1 = 0.0, l2 = 0.0, ssim_ch[3];
  for (int ch = 0; ch < 3; ++ch) {
    const double* s = ws + ((size_t)n * 3 + ch) * n_slots * kMetSlot;
    double a = 0.0, b = 0.0, q = 0.0;
    for (int k = lane; k < n_slots; k += 64) {
      a += s[(size_t)k * kMetSlot];
      b += s[(size_t)k * kMetSlot + 1];
      q += s[(size_t)k * kMetSlot + 2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      b += __shfl_xor(b, o, 64);
      q += __shfl_xor(q, o, 64);
    }
    l1 += a;
    l2 += b;
    ssim_ch[ch] = q / ((double)(H - 2 * kMetHalo) * (double)(W - 2 * kMetHalo));
  }
  if (lane == 0) {
    const double npx = 3.0 * (double)H * (double)W;
    const double mse = l2 / npx;
    double* o = out + (size_t)n * 4;
    o[0] = l1 / npx;
    o[1] = mse;
    o[2] = 10.0 * log10(1.0 / mse);              // +inf when mse == 0, as skimage returns
    o[3] = (ssim_ch[0] + ssim_ch[1] + ssim_ch[2]) / 3.0;
  }
}

int metrics_grid(int N, int H, int W, dim3* grid, int* n_tiles) {
  const long long nb = (H + kMetBand - 1) / kMetBand, nt = (W + kMetTileW - 1) / kMetTileW;
  if (nb * nt > 0x7fffffffLL || N > 65535) return DINER_E_INVALID;
  *grid = dim3((unsigned)(nb * nt), 3, (unsigned)N);
  *n_tiles = (int)nt;
  return 0;
}

int check_metrics_args(const void* pred, const void* gt, int N, int H, int W, int pred_c, int gt_c, const void* ws, const void* out,
                       const char* who) {
  DINER_CHECK_ARG(pred && gt && ws && out, "%s: null pointer argument", who);
  DINER_CHECK_ARG(N >= 1 && N <= 65535, "%s: N = %d images, need 1 <= N <= 65535", who, N);
  DINER_CHECK_ARG(H >= 7 && W >= 7, "%s: %d x %d image: H and W must be at least 7 (the SSIM window)", who, H, W);
  DINER_CHECK_ARG(H <= 65536 && W <= 65536, "%s: %d x %d image: H and W must be at most 65536", who, H, W);
  DINER_CHECK_ARG(pred_c == 3, "%s: pred has %d channels, need 3", who, pred_c);
  DINER_CHECK_ARG(gt_c == 3 || gt_c == 4, "%s: gt has %d channels, need 3 or 4 (alpha is dropped)", who, gt_c);
  return 0;
}

template <class Src>
int launch_metrics(const Src& src, int N, int H, int W, void* workspace, double* out, void* stream) {
  dim3 grid;
  int n_tiles = 0;
  metrics_grid(N, H, W, &grid, &n_tiles);
  hipLaunchKernelGGL(k_metrics_partial<Src>, grid, dim3(kMetThreads), 0, (hipStream_t)stream, src, H, W, n_tiles,
                     (double*)workspace);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_metrics_finalize, dim3(N), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, (int)grid.x, H, W,
                     out);
  DINER_LAUNCH_OK();
  return 0;
}

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" size_t diner_image_metrics_workspace_bytes(int N, int H, int W) {
  dim3 grid;
  int n_tiles = 0;
  if (N < 1 || H < 7 || W < 7 || H > 65536 || W > 65536 || metrics_grid(N, H, W, &grid, &n_tiles) != 0) return 0;
  return (size_t)N * 3 * grid.x * kMetSlot * sizeof(double);
}

extern "C" int diner_image_metrics_u8(const unsigned char* pred, const unsigned char* gt, int N, int H, int W, int pred_c, int gt_c,
                                      void* workspace, double* out, void* stream) {
  const int rc = check_metrics_args(pred, gt, N, H, W, pred_c, gt_c, workspace, out, "image_metrics_u8");
  if (rc) return rc;
  return launch_metrics(SrcU8{pred, gt, pred_c, gt_c}, N, H, W, workspace, out, stream);
}

extern "C" int diner_image_metrics_f32(const float* pred, const float* gt, int N, int H, int W, void* workspace, double* out,
                                       void* stream) {
  const int rc = check_metrics_args(pred, gt, N, H, W, 3, 3, workspace, out, "image_metrics_f32");
  if (rc) return rc;
  return launch_metrics(SrcF32{pred, gt}, N, H, W, workspace, out, stream);
}
