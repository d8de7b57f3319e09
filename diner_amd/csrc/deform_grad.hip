// The backward pass of deform.hip's modulated deformable 3 x 3 convolution (relu = 0), activations channels-last fp32:
//   y[p,o] = bias[o] + sum_k sum_c w[o,c,k] col[p,k,c],   col[p,k,c] = m S(x[..,c], py, px),   m = sigmoid(offmask[p,18 + k])
// with the sample S, its four corners and its coordinate as deform_geom.hpp states them.  From the upstream gradient dy (N,H,W,Cout):
//   G[p,k,c]      = sum_o dy[p,o] w[o,c,k]
//   d_logit[p,k]  = m (1 - m) sum_c G S
//   d_dy[p,k]     = m sum_c G (gy0 v00 + gy1 v01 + gy2 v10 + gy3 v11)         gy, gx: deform_corner_grads(); a corner that is not valid
//   d_dx[p,k]     = m sum_c G (gx0 v00 + gx1 v01 + gx2 v10 + gx3 v11)         counts as 0
//   d_x[idx_i,c] += m wt_i G[p,k,c]                                           for every valid corner i
//   d_weight[o,c,k] = sum_p dy[p,o] col[p,k,c],   d_bias[o] = sum_p dy[p,o]
// A tap that deform_corners() puts outside (a NaN, infinite or huge offset included) reads nothing and every gradient of it is exactly 0.
//
// k_deform_grad_data (d_offmask, d_x).  A workgroup (four waves) takes 64 consecutive pixels of ONE image, as the forward does; dy's tile
// is staged in LDS once.  Per tap:
//   1. the tap's weights w[:, :, k] go to LDS as [o][c];
//   2. wave v forms G for pixels 16 v .. 16 v + 15 on v_mfma_f32_16x16x4_f32 (K = the output channels, ascending) and leaves it in LDS;
//   3. thread t samples pixel t >> 2 for its quarter of the channels (the forward's roles): the three dot products over c are partial sums
//      in registers in the order c ascending within the thread's float4s, and the four threads of a pixel add them as
//      (q0 + q1) + (q2 + q3) by two xor shuffles.  d_offmask is written once per element: no atomics, no memset, the same bits on every
//      run and at any batch position.  The pixel's four corner indices and m wt_i go to LDS;
//   4. the scatter: wave v walks the 64 (pixel, corner) rows of its 16 pixels, a lane a channel -- one instruction adds 64 / Cin
//      contiguous rows of Cin floats with native float atomics.  d_x is zeroed by the entry first.  The order of the adds is not fixed,
//      so d_x alone is not bit-reproducible.
// k_deform_grad_weight (d_weight, d_bias).  Workgroup (s, k) walks the tiles s, s + S, s + 2 S, ... of all images for tap k, samples the
// tap's column matrix again (the forward's arithmetic, bit for bit) into LDS beside dy's tile and adds dy^T col on the matrix cores with
// the 64 pixels as K; its Cout x Cin accumulators stay in registers over the whole walk (at most 16 a thread).  Tap 0's workgroups also
// add dy's columns for d_bias.  Each workgroup writes one slab; k_deform_grad_finish adds the S slabs of every element in slab order in
// double and rounds once.  S depends on the shape alone (or is forced by the caller), so d_weight and d_bias have the same bits on every run.
#include "common.hpp"
#include "deform_geom.hpp"

namespace diner {
namespace {

constexpr int kDgPix = 64;
constexpr int kDgThreads = 256;
constexpr int kDgMaxC = DINER_DEFORM_MAX_CIN;       // 64: the most input channels, and the most output channels of the backward pass
constexpr int kDgTaps = 9;
constexpr int kDgRow = kDgMaxC + 4;                 // words a pixel's row of dy and G: 17 float4s, so 16 pixels x 4 k cover the 64 banks once
constexpr int kDgOp = kDgMaxC + 16;                 // words a row of a B operand read four k rows at a time: they start 16 banks apart
constexpr int kDgMaxSlabs = 1024;
constexpr int kDgDefaultSlabs = 128;

struct DeformGradArgs {
  const float* x;        // (N,H,W,Cin)
  const float* om;       // (N,H,W,27)
  const float* w;        // (Cout,Cin,3,3)
  const float* dy;       // (N,H,W,Cout)
  float* d_x;            // (N,H,W,Cin) zeroed, or null
  float* d_om;           // (N,H,W,27) or null
  float* slab;           // [S][9 Cout Cin + Cout]
  int H, W, Cin, Cout, tiles_per_image, tiles, S, want_w;
};

__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

template <int CV>
__global__ __launch_bounds__(kDgThreads) void k_deform_grad_data(DeformGradArgs a) {
  __shared__ __attribute__((aligned(16))) float Ds[kDgPix * kDgRow];
  __shared__ __attribute__((aligned(16))) float Gs[kDgPix * kDgRow];
  __shared__ __attribute__((aligned(16))) float Wk[kDgMaxC * kDgOp];
  __shared__ float Cf[kDgPix * 4];
  __shared__ int Ci[kDgPix * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
  const int HW = a.H * a.W, Cin = a.Cin, Cout = a.Cout;
  const int Kp = (Cout + 3) & ~3, Np = (Cin + 15) & ~15;
  const int p0 = (int)blockIdx.x * kDgPix;
  const size_t img = blockIdx.y;
  const float* x = a.x + img * HW * Cin;
  const float* om = a.om + img * HW * 27;
  const float* dy = a.dy + img * HW * Cout;
  const int sp = tid >> 2, sq = tid & 3, spix = p0 + sp;
  const bool live = spix < HW;
  const int sh = live ? spix / a.W : 0, sw = live ? spix % a.W : 0;
  const int c4n = Cin >> 2;

  for (int e = tid; e < kDgPix * Kp; e += kDgThreads) {
    const int p = e / Kp, o = e - p * Kp;
    Ds[p * kDgRow + o] = (p0 + p < HW && o < Cout) ? dy[(size_t)(p0 + p) * Cout + o] : 0.0f;
  }

  for (int k = 0; k < kDgTaps; ++k) {
    for (int e = tid; e < Kp * Np; e += kDgThreads) {
      const int o = e / Np, c = e - o * Np;
      Wk[o * kDgOp + c] = (o < Cout && c < Cin) ? a.w[((size_t)o * Cin + c) * kDgTaps + k] : 0.0f;
    }
    __syncthreads();
    // G: rows the wave's 16 pixels, K the output channels, 16 input channels a column tile
    for (int j = 0; j < Np / 16; ++j) {
      v4f acc = (v4f){0.f, 0.f, 0.f, 0.f};
      const float* arow = &Ds[(16 * wave + lc) * kDgRow + lk];
      for (int kk = 0; kk < Kp; kk += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[kk], Wk[(kk + lk) * kDgOp + 16 * j + lc], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) Gs[(16 * wave + 4 * lk + r) * kDgRow + 16 * j + lc] = acc[r];
    }
    __syncthreads();

    DeformCornerGrads g = deform_corner_grads(0, 0, 0, 0, -2.0f, -2.0f, 1, 1);       // outside: nothing valid, every weight 0
    float m = 0.0f;
    if (live) {
      const float* o = om + (size_t)spix * 27;
      g = deform_corner_grads(sh, sw, k / 3, k % 3, o[2 * k], o[2 * k + 1], a.H, a.W);
      m = sigmoidf(o[18 + k]);
    }
    if (a.d_om) {
      float sS = 0.0f, sY = 0.0f, sX = 0.0f;
#pragma unroll
      for (int u = 0; u < CV; ++u) {
        const int c4 = sq + 4 * u;
        if (c4 < c4n) {
          v4f v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[i] = (v4f){0.f, 0.f, 0.f, 0.f};
            if ((g.c.valid >> i) & 1u) v[i] = *reinterpret_cast<const v4f*>(x + (size_t)g.c.idx[i] * Cin + 4 * c4);
          }
          const v4f G4 = *reinterpret_cast<const v4f*>(&Gs[sp * kDgRow + 4 * c4]);
          const v4f S4 = ((g.c.wt[0] * v[0] + g.c.wt[1] * v[1]) + g.c.wt[2] * v[2]) + g.c.wt[3] * v[3];
          const v4f Y4 = ((g.gy[0] * v[0] + g.gy[1] * v[1]) + g.gy[2] * v[2]) + g.gy[3] * v[3];
          const v4f X4 = ((g.gx[0] * v[0] + g.gx[1] * v[1]) + g.gx[2] * v[2]) + g.gx[3] * v[3];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            sS = fmaf(G4[j], S4[j], sS);
            sY = fmaf(G4[j], Y4[j], sY);
            sX = fmaf(G4[j], X4[j], sX);
          }
        }
      }
      sS += __shfl_xor(sS, 1);
      sY += __shfl_xor(sY, 1);
      sX += __shfl_xor(sX, 1);
      sS += __shfl_xor(sS, 2);
      sY += __shfl_xor(sY, 2);
      sX += __shfl_xor(sX, 2);
      if (live && sq == 0) {
        float* o = a.d_om + (img * HW + spix) * 27;
        o[2 * k] = m * sY;
        o[2 * k + 1] = m * sX;
        o[18 + k] = (m * (1.0f - m)) * sS;
      }
    }
    if (a.d_x) {
      // thread sq of the pixel publishes corner sq (selected without indexing a register array by a runtime value)
      const float wt = sq == 0 ? g.c.wt[0] : sq == 1 ? g.c.wt[1] : sq == 2 ? g.c.wt[2] : g.c.wt[3];
      const int id = sq == 0 ? g.c.idx[0] : sq == 1 ? g.c.idx[1] : sq == 2 ? g.c.idx[2] : g.c.idx[3];
      const bool ok = live && ((g.c.valid >> sq) & 1u);
      Cf[tid] = ok ? m * wt : 0.0f;
      Ci[tid] = ok ? id : 0;
      __syncthreads();
      float* dx = a.d_x + img * HW * Cin;
      const int per = 64 / Cin, se = lane / Cin, sc = lane - se * Cin;      // rows of Cin floats one wave instruction adds
      if (se < per) {
        for (int r = se; r < 64; r += per) {
          const int row = 64 * wave + r;                                   // = 4 (pixel of the tile) + corner
          const float cf = Cf[row];
          if (cf != 0.0f) unsafeAtomicAdd(dx + (size_t)Ci[row] * Cin + sc, cf * Gs[(row >> 2) * kDgRow + sc]);
        }
      }
    }
    __syncthreads();                    // Gs, Wk, Cf and Ci are rewritten by the next tap
  }
}

template <int CV>
__global__ __launch_bounds__(kDgThreads) void k_deform_grad_weight(DeformGradArgs a) {
  __shared__ __attribute__((aligned(16))) float Ds[kDgPix * kDgOp];
  __shared__ __attribute__((aligned(16))) float Cs[kDgPix * kDgOp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
  const int HW = a.H * a.W, Cin = a.Cin, Cout = a.Cout;
  const int Mp = (Cout + 15) & ~15, Np = (Cin + 15) & ~15, NT = Np / 16, T = (Mp / 16) * NT;
  const int s = blockIdx.x, k = blockIdx.y;
  const int sp = tid >> 2, sq = tid & 3;
  const int c4n = Cin >> 2, c4p = Np >> 2;
  v4f acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (v4f){0.f, 0.f, 0.f, 0.f};
  double bacc = 0.0;                    // d_bias: this thread's column of dy over the whole walk, rounded once into the slab

  for (int tile = s; tile < a.tiles; tile += a.S) {
    const size_t img = tile / a.tiles_per_image;
    const int p0 = (tile - (int)img * a.tiles_per_image) * kDgPix;
    const float* dy = a.dy + img * HW * Cout;
    for (int e = tid; e < kDgPix * Mp; e += kDgThreads) {
      const int p = e / Mp, o = e - p * Mp;
      Ds[p * kDgOp + o] = (p0 + p < HW && o < Cout) ? dy[(size_t)(p0 + p) * Cout + o] : 0.0f;
    }
    if (a.want_w) {
      const float* x = a.x + img * HW * Cin;
      const int spix = p0 + sp;
      const bool live = spix < HW;
      DeformCorners c = deform_corners(0, 0, 0, 0, -2.0f, -2.0f, 1, 1);
      float m = 0.0f;
      if (live) {
        const float* o = a.om + (img * HW + spix) * 27;
        c = deform_corners(spix / a.W, spix % a.W, k / 3, k % 3, o[2 * k], o[2 * k + 1], a.H, a.W);
        m = sigmoidf(o[18 + k]);
      }
#pragma unroll
      for (int u = 0; u < CV; ++u) {
        const int c4 = sq + 4 * u;
        if (c4 < c4p) {
          v4f val = (v4f){0.f, 0.f, 0.f, 0.f};
          if (c4 < c4n) {
            v4f v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              v[i] = (v4f){0.f, 0.f, 0.f, 0.f};
              if ((c.valid >> i) & 1u) v[i] = *reinterpret_cast<const v4f*>(x + (size_t)c.idx[i] * Cin + 4 * c4);
            }
            val = (((c.wt[0] * v[0] + c.wt[1] * v[1]) + c.wt[2] * v[2]) + c.wt[3] * v[3]) * m;
          }
          *reinterpret_cast<v4f*>(&Cs[sp * kDgOp + 4 * c4]) = val;
        }
      }
    }
    __syncthreads();
    if (a.want_w) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = wave + 4 * i;
        if (j < T) {
          const int mo = j / NT, nc = j - mo * NT;
          for (int kk = 0; kk < kDgPix; kk += 4)
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ds[(kk + lk) * kDgOp + 16 * mo + lc], Cs[(kk + lk) * kDgOp + 16 * nc + lc], acc[i], 0, 0, 0);
        }
      }
    }
    if (k == 0 && tid < Cout)
      for (int p = 0; p < kDgPix; ++p) bacc += (double)Ds[p * kDgOp + tid];
    __syncthreads();
  }

  float* sl = a.slab + (size_t)s * (kDgTaps * Cout * Cin + Cout);
  if (a.want_w) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = wave + 4 * i;
      if (j < T) {
        const int mo = j / NT, nc = j - mo * NT, c = 16 * nc + lc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = 16 * mo + 4 * lk + r;
          if (o < Cout && c < Cin) sl[((size_t)k * Cout + o) * Cin + c] = acc[i][r];
        }
      }
    }
  }
  if (k == 0 && tid < Cout) sl[kDgTaps * Cout * Cin + tid] = (float)bacc;
}

// one thread an element: the S slabs in slab order, in double, rounded once
__global__ __launch_bounds__(256) void k_deform_grad_finish(const float* __restrict__ slab, float* __restrict__ d_w, float* __restrict__ d_b, int Cin,
                                                             int Cout, int S) {
  const int nw = kDgTaps * Cout * Cin, per = nw + Cout;
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= per) return;
  if (e < nw ? d_w == nullptr : d_b == nullptr) return;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += (double)slab[(size_t)s * per + e];
  if (e < nw) {
    const int k = e / (Cout * Cin), o = (e / Cin) % Cout, c = e % Cin;
    d_w[((size_t)o * Cin + c) * kDgTaps + k] = (float)sum;
  } else {
    d_b[e - nw] = (float)sum;
  }
}

template <int CV>
void launch_grad(const DeformGradArgs& a, int N, bool data, bool weight, hipStream_t stream) {
  if (data) hipLaunchKernelGGL((k_deform_grad_data<CV>), dim3((unsigned)a.tiles_per_image, (unsigned)N), dim3(kDgThreads), 0, stream, a);
  if (weight) hipLaunchKernelGGL((k_deform_grad_weight<CV>), dim3((unsigned)a.S, a.want_w ? kDgTaps : 1), dim3(kDgThreads), 0, stream, a);
}

bool grad_limits(int N, int H, int W, int Cin, int Cout) {
  return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= (1 << 14) && W <= (1 << 14) && Cin >= 8 && Cin <= kDgMaxC && Cin % 8 == 0 && Cout >= 1 &&
         Cout <= kDgMaxC && (long long)N * ((H * W + kDgPix - 1) / kDgPix) < (1LL << 30);
}

int grad_slabs(int N, int H, int W, int slabs) {
  const long long tiles = (long long)N * ((H * W + kDgPix - 1) / kDgPix);
  const long long want = slabs > 0 ? (slabs < kDgMaxSlabs ? slabs : kDgMaxSlabs) : kDgDefaultSlabs;
  return (int)(want < tiles ? want : tiles);
}

}  // namespace
}  // namespace diner

using namespace diner;

extern "C" size_t diner_deform_conv3x3_grad_workspace_floats(int N, int H, int W, int Cin, int Cout, int slabs) {
  if (!grad_limits(N, H, W, Cin, Cout) || slabs < 0) return 0;
  return (size_t)grad_slabs(N, H, W, slabs) * ((size_t)kDgTaps * Cout * Cin + Cout);
}

extern "C" int diner_deform_conv3x3_grad_f32(const float* x, const float* offmask, const float* weight, const float* dy, float* d_x, float* d_offmask,
                                             float* d_weight, float* d_bias, float* workspace, int N, int H, int W, int Cin, int Cout, int slabs,
                                             void* stream) {
  int rc = check_nhwc("deform_conv3x3_grad", N, H, W, Cin);
  if (rc) return rc;
  DINER_CHECK_ARG(Cin >= 8 && Cin <= kDgMaxC && Cin % 8 == 0, "deform_conv3x3_grad: Cin = %d (a multiple of 8 in [8, %d])", Cin, kDgMaxC);
  DINER_CHECK_ARG(Cout >= 1 && Cout <= kDgMaxC, "deform_conv3x3_grad: Cout = %d (must be in [1, %d])", Cout, kDgMaxC);
  DINER_CHECK_ARG(N <= 65535, "deform_conv3x3_grad: N = %d images (at most 65535 a call)", N);
  DINER_CHECK_ARG(H <= (1 << 14) && W <= (1 << 14), "deform_conv3x3_grad: H, W = %d, %d (each at most 2^14)", H, W);
  DINER_CHECK_ARG(grad_limits(N, H, W, Cin, Cout), "deform_conv3x3_grad: %d x %d x %d pixels are too many tiles", N, H, W);
  DINER_CHECK_ARG(slabs >= 0, "deform_conv3x3_grad: slabs = %d (0 for the default, or a positive count)", slabs);
  DINER_CHECK_ARG(x && offmask && weight && dy, "deform_conv3x3_grad: null input pointer");
  DINER_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0, "deform_conv3x3_grad: x must be 16-byte aligned");
  DINER_CHECK_ARG(((reinterpret_cast<uintptr_t>(offmask) | reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(dy) |
                    reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_offmask) | reinterpret_cast<uintptr_t>(d_weight) |
                    reinterpret_cast<uintptr_t>(d_bias) | reinterpret_cast<uintptr_t>(workspace)) & 3) == 0,
                  "deform_conv3x3_grad: every pointer must be 4-byte aligned");
  const bool data = d_x || d_offmask, wb = d_weight || d_bias;
  DINER_CHECK_ARG(!wb || workspace, "deform_conv3x3_grad: d_weight and d_bias need the workspace (diner_deform_conv3x3_grad_workspace_floats)");
  DINER_CHECK_ARG(!d_x || (d_x != x && d_x != dy && d_x != offmask), "deform_conv3x3_grad: d_x must not be one of the inputs");
  DINER_CHECK_ARG(!d_offmask || (d_offmask != x && d_offmask != dy && d_offmask != offmask),
                  "deform_conv3x3_grad: d_offmask must not be one of the inputs");
  if (!data && !wb) return 0;
  DeformGradArgs a;
  a.x = x; a.om = offmask; a.w = weight; a.dy = dy; a.d_x = d_x; a.d_om = d_offmask; a.slab = workspace;
  a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.tiles_per_image = (H * W + kDgPix - 1) / kDgPix;
  a.tiles = N * a.tiles_per_image;
  a.S = grad_slabs(N, H, W, slabs);
  a.want_w = d_weight != nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (d_x) DINER_HIP_OK(hipMemsetAsync(d_x, 0, (size_t)N * H * W * Cin * sizeof(float), st));
  const int cv = Cin <= 16 ? 1 : Cin <= 32 ? 2 : 4;
  (cv == 1 ? launch_grad<1> : cv == 2 ? launch_grad<2> : launch_grad<4>)(a, N, data, wb, st);
  DINER_LAUNCH_OK();
  if (wb) {
    const int per = kDgTaps * Cout * Cin + Cout;
    hipLaunchKernelGGL(k_deform_grad_finish, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, workspace, d_weight, d_bias, Cin, Cout, a.S);
    DINER_LAUNCH_OK();
  }
  return 0;
}
