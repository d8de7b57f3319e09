// The matching stage of the multi-view depth estimator (TransMVSNet's DepthNet.forward between its learned networks): the cost volume
// of one reference view against NS source views, the winner-take-all read-out of the regularised cost, and the next stage's depth
// hypotheses; and for training the per-view similarity with its backward pass at the feature maps (k_mvs_similarity, k_mvs_similarity_grad).
// Layouts, limits and operation order are documented in include/diner_hip.h.
//
// k_mvs_cost_volume never forms the warped (B,C,D,H,W) volume or a sampling grid: a thread owns (pixel, every DL-th depth), keeps the
// reference pixel's C features in registers across depths and views, gathers the four bilinear taps of a sample as 16-byte loads from
// the channels-last source map and writes one similarity.  A view's D similarities wait in an LDS slab until that view's weight
// max_d sigmoid(net(similarity_d)) is known, then enter the weighted sum held in a second slab; both slabs are D x PB floats, and PB
// (pixels per workgroup) is chosen from D so that the two fit 32 KiB -- one code path.  Every element of either slab is read and written
// by one thread only; the only exchange between threads is the maximum over a pixel's DL partial maxima.  No atomics, the order of every
// sum is fixed by the shape alone, no tile crosses samples of the batch.
#include "common.hpp"
#include "mvs_geom.hpp"

namespace diner {

namespace {

constexpr int kMvsThreads = 256;
constexpr int kMvsSlabBytes = 32 * 1024;        // both slabs together
constexpr int kMvsNetFloats = DINER_MVS_PIXELWISE_FLOATS;
constexpr int kMvsMaxD = DINER_MVS_MAX_DEPTHS;
constexpr int kMvsMaxC = DINER_MVS_MAX_CHANNELS;

// One thread per (sample b, source view v): rot | trans of (K_s E_s[:3] ; 0 0 0 1) inverse(K_r E_r[:3] ; 0 0 0 1) in double, rounded once.
// With P = [A t ; 0 1]: P_s inverse(P_r) = [A_s inverse(A_r), t_s - A_s inverse(A_r) t_r ; 0 1]; inverse(A_r) by the adjugate.
__global__ void k_mvs_homography(const float* __restrict__ proj, float* __restrict__ hom, int B, int NS) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * NS) return;
  const int b = i / NS, v = i - b * NS;
  const float* pr = proj + (size_t)(b * (NS + 1)) * 32;
  const float* ps = proj + (size_t)(b * (NS + 1) + v + 1) * 32;
  double Ar[3][3], tr[3], As[3][3], ts[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c) {
      double sr = 0.0, ss = 0.0;
      for (int k = 0; k < 3; ++k) {              // K[:3,:3] E[:3,:4]; K is the second 4x4 of the pair
        sr += (double)pr[16 + r * 4 + k] * (double)pr[k * 4 + c];
        ss += (double)ps[16 + r * 4 + k] * (double)ps[k * 4 + c];
      }
      if (c < 3) { Ar[r][c] = sr; As[r][c] = ss; } else { tr[r] = sr; ts[r] = ss; }
    }
  }
  double adj[3][3];
  adj[0][0] = Ar[1][1] * Ar[2][2] - Ar[1][2] * Ar[2][1];
  adj[0][1] = Ar[0][2] * Ar[2][1] - Ar[0][1] * Ar[2][2];
  adj[0][2] = Ar[0][1] * Ar[1][2] - Ar[0][2] * Ar[1][1];
  adj[1][0] = Ar[1][2] * Ar[2][0] - Ar[1][0] * Ar[2][2];
  adj[1][1] = Ar[0][0] * Ar[2][2] - Ar[0][2] * Ar[2][0];
  adj[1][2] = Ar[0][2] * Ar[1][0] - Ar[0][0] * Ar[1][2];
  adj[2][0] = Ar[1][0] * Ar[2][1] - Ar[1][1] * Ar[2][0];
  adj[2][1] = Ar[0][1] * Ar[2][0] - Ar[0][0] * Ar[2][1];
  adj[2][2] = Ar[0][0] * Ar[1][1] - Ar[0][1] * Ar[1][0];
  const double det = Ar[0][0] * adj[0][0] + Ar[0][1] * adj[1][0] + Ar[0][2] * adj[2][0];
  float* o = hom + (size_t)i * 12;
  for (int r = 0; r < 3; ++r) {
    double rot[3];
    for (int c = 0; c < 3; ++c) rot[c] = (As[r][0] * adj[0][c] + As[r][1] * adj[1][c] + As[r][2] * adj[2][c]) / det;
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = (float)rot[c];
    o[9 + r] = (float)(ts[r] - (rot[0] * tr[0] + rot[1] * tr[1] + rot[2] * tr[2]));
  }
}

// sigmoid(conv2(relu(conv1(relu(conv0(s)))))) of the 1 -> 16 -> 8 -> 1 pointwise net, BatchNorm folded.  net (LDS):
// w0[16] b0[16] w1[8][16] b1[8] w2[8] b2; every sum is an fmaf chain that starts at the bias and runs over the inputs in order.
__device__ __forceinline__ float pixelwise_weight(const float* net, float s) {
  float h0[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) h0[j] = fmaxf(__fmaf_rn(net[j], s, net[16 + j]), 0.0f);
  float y = net[32 + 128 + 8 + 8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float a = net[32 + 128 + k];
#pragma unroll
    for (int j = 0; j < 16; ++j) a = __fmaf_rn(net[32 + k * 16 + j], h0[j], a);
    y = __fmaf_rn(net[32 + 128 + 8 + k], fmaxf(a, 0.0f), y);
  }
  return 1.0f / (1.0f + expf(-y));
}

struct MvsArgs {
  const float* ref_cl;        // (B,H,W,C)
  const float* src_cl;        // (NS,B,H,W,C)
  const float* hom;           // (B,NS,12)
  const float* depth;         // (B,D,H,W)
  const float* net;           // kMvsNetFloats or null
  const float* vw_in;         // (B,NS,H,W) or null
  float* sim;                 // (B,D,H,W)
  float* vw_out;              // (B,NS,H,W) or null
  int B, NS, D, H, W, PB, blocks_per_sample;
};

// dot of tap (xi, yi)'s C features with the reference features; out-of-map taps read a clamped address and are zeroed by the caller's weight
template <int C4>
__device__ __forceinline__ float tap_dot(const float4* __restrict__ map, int xi, int yi, int W, const float4 (&rf)[C4]) {
  const float4* t = map + ((size_t)yi * W + xi) * C4;
  float a = 0.0f;
#pragma unroll
  for (int c = 0; c < C4; ++c) {
    const float4 f = t[c];
    a = __fmaf_rn(f.x, rf[c].x, a);
    a = __fmaf_rn(f.y, rf[c].y, a);
    a = __fmaf_rn(f.z, rf[c].z, a);
    a = __fmaf_rn(f.w, rf[c].w, a);
  }
  return a;
}

template <int C4>
__global__ void __launch_bounds__(kMvsThreads) k_mvs_cost_volume(MvsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int PB = a.PB, DL = kMvsThreads / PB, D = a.D, H = a.H, W = a.W;
  float* slab = lds;                             // [D][PB] this view's similarities
  float* acc = lds + (size_t)D * PB;             // [D][PB] sum_v similarity_v w_v
  float* red = acc + (size_t)D * PB;             // [DL][PB] partial maxima
  float* net = red + kMvsThreads;                // kMvsNetFloats
  const int tid = threadIdx.x;
  const int p = tid % PB, dl = tid / PB;
  const int b = blockIdx.x / a.blocks_per_sample;
  const int pix = (blockIdx.x - b * a.blocks_per_sample) * PB + p;
  const int HW = H * W;
  const bool live = pix < HW;
  const int pc = live ? pix : HW - 1;            // dead lanes compute on the last pixel and write nothing
  const int y = pc / W, x = pc - y * W;
  if (a.net != nullptr)
    for (int i = tid; i < kMvsNetFloats; i += kMvsThreads) net[i] = a.net[i];
  for (int d = dl; d < D; d += DL) acc[d * PB + p] = 0.0f;

  float4 rf[C4];
  {
    const float4* r = reinterpret_cast<const float4*>(a.ref_cl) + ((size_t)b * HW + pc) * C4;
#pragma unroll
    for (int c = 0; c < C4; ++c) rf[c] = r[c];
  }
  const float fx = (float)x, fy = (float)y;
  const float fc = (float)(4 * C4);
  const float* dep = a.depth + (size_t)b * D * HW + pc;
  float wsum = 1e-5f;
  __syncthreads();                               // net[] is staged

  for (int v = 0; v < a.NS; ++v) {
    const float* hm = a.hom + ((size_t)b * a.NS + v) * 12;
    const float4* map = reinterpret_cast<const float4*>(a.src_cl) + ((size_t)v * a.B + b) * HW * C4;
    // rot (x, y, 1): the same three values for every depth
    const float rx = __fmaf_rn(hm[1], fy, __fmul_rn(hm[0], fx)) + hm[2];
    const float ry = __fmaf_rn(hm[4], fy, __fmul_rn(hm[3], fx)) + hm[5];
    const float rz = __fmaf_rn(hm[7], fy, __fmul_rn(hm[6], fx)) + hm[8];
    float wmax = 0.0f;                           // the maximum of sigmoids, which are >= 0
    for (int d = dl; d < D; d += DL) {
      const float z = dep[(size_t)d * HW];
      const float px3 = __fmaf_rn(rx, z, hm[9]), py3 = __fmaf_rn(ry, z, hm[10]), pz3 = __fmaf_rn(rz, z, hm[11]);
      const bool valid = !(pz3 < 1e-6f);
      // beyond [-1, size] every tap is outside; the clamp keeps the conversion to int defined and sends NaN to "outside"
      const float sx = fminf(fmaxf(px3 / pz3, -2.0f), (float)W + 1.0f);
      const float sy = fminf(fmaxf(py3 / pz3, -2.0f), (float)H + 1.0f);
      const float x0f = floorf(sx), y0f = floorf(sy);
      const int x0 = (int)x0f, y0 = (int)y0f;
      const float tx = sx - x0f, ty = sy - y0f;
      const bool inx0 = x0 >= 0 && x0 < W, inx1 = x0 + 1 >= 0 && x0 + 1 < W;
      const bool iny0 = y0 >= 0 && y0 < H, iny1 = y0 + 1 >= 0 && y0 + 1 < H;
      const float wx0 = (valid && inx0) ? 1.0f - tx : 0.0f, wx1 = (valid && inx1) ? tx : 0.0f;
      const float wy0 = iny0 ? 1.0f - ty : 0.0f, wy1 = iny1 ? ty : 0.0f;
      const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
      const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
      const float t00 = tap_dot<C4>(map, xa, ya, W, rf), t01 = tap_dot<C4>(map, xb, ya, W, rf);
      const float t10 = tap_dot<C4>(map, xa, yb, W, rf), t11 = tap_dot<C4>(map, xb, yb, W, rf);
      float s = __fmul_rn(__fmul_rn(wx0, wy0), t00);
      s = __fmaf_rn(__fmul_rn(wx1, wy0), t01, s);
      s = __fmaf_rn(__fmul_rn(wx0, wy1), t10, s);
      s = __fmaf_rn(__fmul_rn(wx1, wy1), t11, s);
      s = s / fc;
      slab[d * PB + p] = s;
      if (a.net != nullptr) wmax = fmaxf(wmax, pixelwise_weight(net, s));
    }
    float w;
    if (a.net != nullptr) {
      red[dl * PB + p] = wmax;
      __syncthreads();
      w = red[p];
      for (int k = 1; k < DL; ++k) w = fmaxf(w, red[k * PB + p]);
      __syncthreads();                           // red[] is rewritten by the next view
      if (dl == 0 && live) a.vw_out[((size_t)b * a.NS + v) * HW + pix] = w;
    } else {
      w = a.vw_in[((size_t)b * a.NS + v) * HW + pc];
    }
    for (int d = dl; d < D; d += DL) acc[d * PB + p] = __fadd_rn(acc[d * PB + p], __fmul_rn(slab[d * PB + p], w));
    wsum = __fadd_rn(wsum, w);
  }
  if (live) {
    float* o = a.sim + (size_t)b * D * HW + pix;
    for (int d = dl; d < D; d += DL) o[(size_t)d * HW] = acc[d * PB + p] / wsum;
  }
}

template <int C4>
void launch_cost_volume(const MvsArgs& a, int grid, size_t lds_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(k_mvs_cost_volume<C4>, dim3(grid), dim3(kMvsThreads), lds_bytes, stream, a);
}

// prob = exp(log_softmax(cost [+ init])) along D, the first index of its maximum, depth = hypotheses[argmax], confidence = prob[argmax]
__global__ void __launch_bounds__(kMvsThreads) k_mvs_select_depth(const float* __restrict__ cost, const float* __restrict__ init,
                                                                  const float* __restrict__ hyp, float* __restrict__ depth,
                                                                  float* __restrict__ conf, float* __restrict__ prob, int total, int D, int HW) {
  const int i = blockIdx.x * kMvsThreads + threadIdx.x;
  if (i >= total) return;
  const int b = i / HW, pix = i - b * HW;
  const size_t base = (size_t)b * D * HW + pix;
  float m = -INFINITY;
  for (int d = 0; d < D; ++d) {
    float c = cost[base + (size_t)d * HW];
    if (init != nullptr) c = __fadd_rn(c, init[base + (size_t)d * HW]);
    m = fmaxf(m, c);
  }
  float sum = 0.0f;
  for (int d = 0; d < D; ++d) {
    float c = cost[base + (size_t)d * HW];
    if (init != nullptr) c = __fadd_rn(c, init[base + (size_t)d * HW]);
    sum = __fadd_rn(sum, expf(__fsub_rn(c, m)));
  }
  const float lse = logf(sum);
  float best = -1.0f;
  int arg = 0;
  for (int d = 0; d < D; ++d) {
    float c = cost[base + (size_t)d * HW];
    if (init != nullptr) c = __fadd_rn(c, init[base + (size_t)d * HW]);
    const float pr = expf(__fsub_rn(__fsub_rn(c, m), lse));
    if (prob != nullptr) prob[base + (size_t)d * HW] = pr;
    if (pr > best) { best = pr; arg = d; }      // strict: the first index of the maximum
  }
  depth[i] = hyp[base + (size_t)arg * HW];
  conf[i] = best;
}

// torch's area_pixel_compute_source_index for align_corners = False: scale (dst + 0.5) - 0.5, clamped at 0; -> lower tap, upper tap, lambda
__device__ __forceinline__ void source_index(float scale, int dst, int in_size, int& i0, int& i1, float& lam) {
  float s = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
  s = fmaxf(s, 0.0f);
  i0 = min((int)s, in_size - 1);
  i1 = min(i0 + 1, in_size - 1);
  lam = fminf(fmaxf(__fsub_rn(s, (float)i0), 0.0f), 1.0f);
}

__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, float lx, float ly) {
  // torch's upsample_bilinear2d: h0lambda (w0lambda v00 + w1lambda v01) + h1lambda (w0lambda v10 + w1lambda v11)
  const float mx = __fsub_rn(1.0f, lx), my = __fsub_rn(1.0f, ly);
  const float top = __fadd_rn(__fmul_rn(mx, v00), __fmul_rn(lx, v01));
  const float bot = __fadd_rn(__fmul_rn(mx, v10), __fmul_rn(lx, v11));
  return __fadd_rn(__fmul_rn(my, top), __fmul_rn(ly, bot));
}

// One thread per output pixel (b, yo, xo) of the (Ho, Wo) hypothesis planes.  The chain it restates: cur (h,w) --bilinear--> (H,W);
// lo = up - half, hi = up + half, step = (hi - lo) / (D - 1), sample_d = lo + d step; --trilinear--> (D, Ho, Wo), which is the identity
// along d and two taps per axis in the plane.
__global__ void __launch_bounds__(kMvsThreads) k_mvs_hypotheses(const float* __restrict__ cur, float* __restrict__ out, int total, int h, int w,
                                                                int H, int W, int Ho, int Wo, int D, float half) {
  const int i = blockIdx.x * kMvsThreads + threadIdx.x;
  if (i >= total) return;
  const int b = i / (Ho * Wo), r = i - b * (Ho * Wo), yo = r / Wo, xo = r - yo * Wo;
  int Y[2], X[2];
  float LY, LX;
  source_index((float)H / (float)Ho, yo, H, Y[0], Y[1], LY);
  source_index((float)W / (float)Wo, xo, W, X[0], X[1], LX);
  const float* c = cur + (size_t)b * h * w;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  float lo[2][2], step[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int y0, y1;
    float ly;
    source_index(sh, Y[j], h, y0, y1, ly);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      int x0, x1;
      float lx;
      source_index(sw, X[k], w, x0, x1, lx);
      const float up = lerp2(c[y0 * w + x0], c[y0 * w + x1], c[y1 * w + x0], c[y1 * w + x1], lx, ly);
      lo[j][k] = __fsub_rn(up, half);
      step[j][k] = __fsub_rn(__fadd_rn(up, half), lo[j][k]) / (float)(D - 1);
    }
  }
  float* o = out + (size_t)b * D * Ho * Wo + r;
  for (int d = 0; d < D; ++d) {
    const float fd = (float)d;
    const float s00 = __fadd_rn(lo[0][0], __fmul_rn(fd, step[0][0])), s01 = __fadd_rn(lo[0][1], __fmul_rn(fd, step[0][1]));
    const float s10 = __fadd_rn(lo[1][0], __fmul_rn(fd, step[1][0])), s11 = __fadd_rn(lo[1][1], __fmul_rn(fd, step[1][1]));
    o[(size_t)d * Ho * Wo] = lerp2(s00, s01, s10, s11, LX, LY);
  }
}

// ---- the per-view similarity and its backward pass (training: diner_amd.mvs.match_similarity / cost_volume_train) ----------------------
// Both kernels keep k_mvs_cost_volume's structure -- a workgroup owns PB pixels of one sample, thread (p, dl) the pixel p and every DL-th
// depth -- and take the tap geometry from mvs_taps (mvs_geom.hpp), which restates that kernel's operations in its order, so
// k_mvs_similarity (the reference pixel's features in registers, like that kernel) writes the bits it keeps in its LDS slab.
struct MvsSimArgs {
  const float* ref_cl;        // (B,H,W,C)
  const float* src_cl;        // (NS,B,H,W,C)
  const float* hom;           // (B,NS,12)
  const float* depth;         // (B,D,H,W)
  float* sim;                 // (B,NS,D,H,W)
  int B, NS, D, H, W, PB, blocks_per_sample;
};

template <int C4>
__device__ __forceinline__ float tap_dot_at(const float4* __restrict__ map, int idx, const float4 (&rf)[C4]) {
  const float4* t = map + (size_t)idx * C4;
  float a = 0.0f;
#pragma unroll
  for (int c = 0; c < C4; ++c) {
    const float4 f = t[c];
    a = __fmaf_rn(f.x, rf[c].x, a);
    a = __fmaf_rn(f.y, rf[c].y, a);
    a = __fmaf_rn(f.z, rf[c].z, a);
    a = __fmaf_rn(f.w, rf[c].w, a);
  }
  return a;
}

template <int C4>
__global__ void __launch_bounds__(kMvsThreads) k_mvs_similarity(MvsSimArgs a) {
  const int PB = a.PB, DL = kMvsThreads / PB, D = a.D, H = a.H, W = a.W;
  const int tid = threadIdx.x;
  const int p = tid % PB, dl = tid / PB;
  const int b = blockIdx.x / a.blocks_per_sample;
  const int pix = (blockIdx.x - b * a.blocks_per_sample) * PB + p;
  const int HW = H * W;
  const bool live = pix < HW;
  const int pc = live ? pix : HW - 1;            // dead lanes compute on the last pixel and write nothing
  const int y = pc / W, x = pc - y * W;
  float4 rf[C4];
  {
    const float4* r = reinterpret_cast<const float4*>(a.ref_cl) + ((size_t)b * HW + pc) * C4;
#pragma unroll
    for (int c = 0; c < C4; ++c) rf[c] = r[c];
  }
  const float fc = (float)(4 * C4);
  const float* dep = a.depth + (size_t)b * D * HW + pc;
  for (int v = 0; v < a.NS; ++v) {
    const float* hm = a.hom + ((size_t)b * a.NS + v) * 12;
    const float4* map = reinterpret_cast<const float4*>(a.src_cl) + ((size_t)v * a.B + b) * HW * C4;
    float* o = a.sim + ((size_t)b * a.NS + v) * D * HW + pc;
    for (int d = dl; d < D; d += DL) {
      const MvsTaps t = mvs_taps(hm, x, y, dep[(size_t)d * HW], H, W);
      const float t00 = tap_dot_at<C4>(map, t.idx[0], rf), t01 = tap_dot_at<C4>(map, t.idx[1], rf);
      const float t10 = tap_dot_at<C4>(map, t.idx[2], rf), t11 = tap_dot_at<C4>(map, t.idx[3], rf);
      float s = __fmul_rn(t.wt[0], t00);
      s = __fmaf_rn(t.wt[1], t01, s);
      s = __fmaf_rn(t.wt[2], t10, s);
      s = __fmaf_rn(t.wt[3], t11, s);
      s = s / fc;
      if (live) o[(size_t)d * HW] = s;
    }
  }
}

struct MvsGradArgs {
  const float* ref_cl;        // (B,H,W,C)
  const float* src_cl;        // (NS,B,H,W,C)
  const float* hom;           // (B,NS,12)
  const float* depth;         // (B,D,H,W)
  const float* g_views;       // (B,NS,D,H,W): the upstream gradient per view, or null
  const float* g_agg;         // (B,D,H,W): the upstream gradient of the aggregated similarity, with vw
  const float* vw;            // (B,NS,H,W)
  float* d_ref;               // (B,H,W,C): every element written
  float* d_src;               // (NS,B,H,W,C): zeroed by the entry, added to atomically
  int B, NS, D, H, W, PB, blocks_per_sample;
};

// d_ref: a thread adds G_vd bw_tap src[v,tap,:] / C over its views, depths and taps into registers; a pixel's DL partial sums meet in LDS
// and are added by one thread in the order dl = 0, 1, ...: no atomics, the order fixed by the shape.  d_src: G_vd bw_tap ref[pixel,:] / C
// goes to each tap's texel by float atomic adds, whose order is not fixed; a tap whose G bw is exactly 0 (outside the map, an invalid
// sample, a masked upstream) is skipped and adds nothing to either.  The adds are issued by the wave together (sample, tap and pixel
// travel by lane shuffles, the reference row is read again, coalesced): a lane a channel, so an instruction adds contiguous rows.
template <int C4>
__global__ void __launch_bounds__(kMvsThreads) k_mvs_similarity_grad(MvsGradArgs a) {
  __shared__ float4 red[kMvsThreads];            // [DL][PB] one float4 of every thread's partial d_ref
  const int PB = a.PB, DL = kMvsThreads / PB, D = a.D, H = a.H, W = a.W;
  const int tid = threadIdx.x;
  const int p = tid % PB, dl = tid / PB;
  const int b = blockIdx.x / a.blocks_per_sample;
  const int pix = (blockIdx.x - b * a.blocks_per_sample) * PB + p;
  const int HW = H * W;
  const bool live = pix < HW;
  const int pc = live ? pix : HW - 1;            // dead lanes compute on the last pixel with a zero upstream: they add and write nothing
  const int y = pc / W, x = pc - y * W;
  float4 acc[C4];
#pragma unroll
  for (int c = 0; c < C4; ++c) acc[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float fc = (float)(4 * C4);
  const float* dep = a.depth + (size_t)b * D * HW + pc;
  constexpr int C = 4 * C4, PER = 64 / C;        // rows of C floats one wave instruction covers
  const int lane = tid & 63, se = lane / C, sc = lane - se * C;
  const float* refb = a.ref_cl + (size_t)b * HW * C;
  float wsum = 1e-5f;                            // the forward's sum, in its order
  if (a.g_views == nullptr)
    for (int v = 0; v < a.NS; ++v) wsum = __fadd_rn(wsum, a.vw[((size_t)b * a.NS + v) * HW + pc]);

  for (int v = 0; v < a.NS; ++v) {
    const float* hm = a.hom + ((size_t)b * a.NS + v) * 12;
    const size_t moff = ((size_t)v * a.B + b) * HW * C4;
    const float4* map = reinterpret_cast<const float4*>(a.src_cl) + moff;
    float* gmap = a.d_src + moff * 4;
    const float w = a.g_views == nullptr ? a.vw[((size_t)b * a.NS + v) * HW + pc] : 0.0f;
    // every lane of a wave runs the same number of rounds (a lane beyond D, a dead lane or a zero upstream carries zero weights), so that
    // the wave can scatter together
    for (int d0 = 0; d0 < D; d0 += DL) {
      const int d = d0 + dl;
      const bool act = live && d < D;
      const int dc = d < D ? d : D - 1;
      float G = 0.0f;
      if (act) {
        if (a.g_views != nullptr) G = a.g_views[(((size_t)b * a.NS + v) * D + dc) * HW + pc];
        else G = __fmul_rn(a.g_agg[((size_t)b * D + dc) * HW + pc], w) / wsum;
      }
      const float Gs = G / fc;
      const MvsTaps t = mvs_taps(hm, x, y, dep[(size_t)dc * HW], H, W);
      float cw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        cw[k] = act ? __fmul_rn(Gs, t.wt[k]) : 0.0f;       // the weights are finite, so a zero upstream gives exact zeros
        if (cw[k] == 0.0f) continue;
        const float4* tp = map + (size_t)t.idx[k] * C4;
#pragma unroll
        for (int c = 0; c < C4; ++c) {
          const float4 f = tp[c];
          acc[c].x = __fmaf_rn(cw[k], f.x, acc[c].x);
          acc[c].y = __fmaf_rn(cw[k], f.y, acc[c].y);
          acc[c].z = __fmaf_rn(cw[k], f.z, acc[c].z);
          acc[c].w = __fmaf_rn(cw[k], f.w, acc[c].w);
        }
      }
      // the scatter: the wave's 64 samples of tap k, PER at a time, a lane a channel -- one instruction adds PER contiguous rows of C
      // floats (neighbouring pixels hit neighbouring texels) instead of 64 lone floats a row apart
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!__any(cw[k] != 0.0f)) continue;               // wave-uniform
        for (int it = 0; it < (64 + PER - 1) / PER; ++it) {
          const int sl = it * PER + se;                    // the lane whose sample this lane helps to add
          const int sidx = __shfl(t.idx[k], sl & 63);
          const float scw = __shfl(cw[k], sl & 63);
          const int spc = __shfl(pc, sl & 63);
          if (se < PER && sl < 64 && scw != 0.0f)
            unsafeAtomicAdd(gmap + (size_t)sidx * C + sc, __fmul_rn(scw, refb[(size_t)spc * C + sc]));
        }
      }
    }
  }
  float4* o = reinterpret_cast<float4*>(a.d_ref) + ((size_t)b * HW + pc) * C4;
#pragma unroll
  for (int c = 0; c < C4; ++c) {
    red[dl * PB + p] = acc[c];
    __syncthreads();
    if (dl == 0 && live) {
      float4 s = red[p];
      for (int k = 1; k < DL; ++k) {
        const float4 q = red[k * PB + p];
        s.x = __fadd_rn(s.x, q.x);
        s.y = __fadd_rn(s.y, q.y);
        s.z = __fadd_rn(s.z, q.z);
        s.w = __fadd_rn(s.w, q.w);
      }
      o[c] = s;
    }
    __syncthreads();                             // red[] is rewritten by the next float4
  }
}

template <int C4>
void launch_similarity(const MvsSimArgs& a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(k_mvs_similarity<C4>, dim3(grid), dim3(kMvsThreads), 0, stream, a);
}

template <int C4>
void launch_similarity_grad(const MvsGradArgs& a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(k_mvs_similarity_grad<C4>, dim3(grid), dim3(kMvsThreads), 0, stream, a);
}

int pixels_per_block(int D) {                    // the LDS slab rule: 2 slabs x D x PB floats <= kMvsSlabBytes, PB a power of two <= 64
  int pb = 64;
  while (pb > 16 && 2 * D * pb * (int)sizeof(float) > kMvsSlabBytes) pb >>= 1;
  return pb;
}

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" int diner_mvs_cost_volume_f32(const float* ref_cl, const float* src_cl, const float* proj, const float* depth, const float* pixelwise,
                                         const float* view_weights_in, float* similarity, float* view_weights_out, float* homography, int B,
                                         int NS, int C, int D, int H, int W, void* stream) {
  DINER_CHECK_ARG(ref_cl && src_cl && proj && depth && similarity && homography, "mvs_cost_volume: null pointer");
  DINER_CHECK_ARG((pixelwise != nullptr) != (view_weights_in != nullptr),
                  "mvs_cost_volume: give either the folded pixelwise net or the view weights, not both and not neither");
  DINER_CHECK_ARG(pixelwise == nullptr || view_weights_out != nullptr, "mvs_cost_volume: computing the view weights needs view_weights_out");
  DINER_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "mvs_cost_volume: B = %d, H = %d, W = %d must be >= 1", B, H, W);
  DINER_CHECK_ARG(NS >= 1 && NS <= DINER_MAX_VIEWS - 1, "mvs_cost_volume: %d source views outside [1, %d]", NS, DINER_MAX_VIEWS - 1);
  DINER_CHECK_ARG(C >= 4 && C <= kMvsMaxC && C % 4 == 0, "mvs_cost_volume: C = %d must be a multiple of 4 in [4, %d]", C, kMvsMaxC);
  DINER_CHECK_ARG(D >= 1 && D <= kMvsMaxD, "mvs_cost_volume: D = %d outside [1, %d]", D, kMvsMaxD);
  DINER_CHECK_ARG((long long)B * D * H * W < (1ll << 31), "mvs_cost_volume: B D H W = %lld must stay below 2^31", (long long)B * D * H * W);
  DINER_CHECK_ARG(((uintptr_t)ref_cl | (uintptr_t)src_cl) % 16 == 0, "mvs_cost_volume: the feature maps must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mvs_homography, dim3((B * NS + 63) / 64), dim3(64), 0, st, proj, homography, B, NS);
  DINER_LAUNCH_OK();
  MvsArgs a;
  a.ref_cl = ref_cl; a.src_cl = src_cl; a.hom = homography; a.depth = depth; a.net = pixelwise; a.vw_in = view_weights_in;
  a.sim = similarity; a.vw_out = view_weights_out;
  a.B = B; a.NS = NS; a.D = D; a.H = H; a.W = W;
  a.PB = pixels_per_block(D);
  a.blocks_per_sample = (H * W + a.PB - 1) / a.PB;
  const long long grid = (long long)a.blocks_per_sample * B;
  DINER_CHECK_ARG(grid < (1ll << 31), "mvs_cost_volume: %lld workgroups", grid);
  const size_t lds_bytes = ((size_t)2 * D * a.PB + kMvsThreads + kMvsNetFloats) * sizeof(float);
  switch (C / 4) {
#define DINER_MVS_CASE(n) case n: launch_cost_volume<n>(a, (int)grid, lds_bytes, st); break;
    DINER_MVS_CASE(1) DINER_MVS_CASE(2) DINER_MVS_CASE(3) DINER_MVS_CASE(4) DINER_MVS_CASE(5) DINER_MVS_CASE(6) DINER_MVS_CASE(7) DINER_MVS_CASE(8)
    DINER_MVS_CASE(9) DINER_MVS_CASE(10) DINER_MVS_CASE(11) DINER_MVS_CASE(12) DINER_MVS_CASE(13) DINER_MVS_CASE(14) DINER_MVS_CASE(15) DINER_MVS_CASE(16)
#undef DINER_MVS_CASE
  }
  DINER_LAUNCH_OK();
  return 0;
}

#define DINER_MVS_LIMITS(who)                                                                                                               \
  DINER_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, who ": B = %d, H = %d, W = %d must be >= 1", B, H, W);                                       \
  DINER_CHECK_ARG(NS >= 1 && NS <= DINER_MAX_VIEWS - 1, who ": %d source views outside [1, %d]", NS, DINER_MAX_VIEWS - 1);                  \
  DINER_CHECK_ARG(C >= 4 && C <= kMvsMaxC && C % 4 == 0, who ": C = %d must be a multiple of 4 in [4, %d]", C, kMvsMaxC);                   \
  DINER_CHECK_ARG(D >= 1 && D <= kMvsMaxD, who ": D = %d outside [1, %d]", D, kMvsMaxD);                                                    \
  DINER_CHECK_ARG((long long)B * D * H * W < (1ll << 31), who ": B D H W = %lld must stay below 2^31", (long long)B * D * H * W)

#define DINER_MVS_DISPATCH(launch, ...)                                                                                                     \
  switch (C / 4) {                                                                                                                          \
    case 1: launch<1>(__VA_ARGS__); break;   case 2: launch<2>(__VA_ARGS__); break;   case 3: launch<3>(__VA_ARGS__); break;                \
    case 4: launch<4>(__VA_ARGS__); break;   case 5: launch<5>(__VA_ARGS__); break;   case 6: launch<6>(__VA_ARGS__); break;                \
    case 7: launch<7>(__VA_ARGS__); break;   case 8: launch<8>(__VA_ARGS__); break;   case 9: launch<9>(__VA_ARGS__); break;                \
    case 10: launch<10>(__VA_ARGS__); break; case 11: launch<11>(__VA_ARGS__); break; case 12: launch<12>(__VA_ARGS__); break;              \
    case 13: launch<13>(__VA_ARGS__); break; case 14: launch<14>(__VA_ARGS__); break; case 15: launch<15>(__VA_ARGS__); break;              \
    case 16: launch<16>(__VA_ARGS__); break;                                                                                                \
  }

extern "C" int diner_mvs_similarity_f32(const float* ref_cl, const float* src_cl, const float* proj, const float* depth, float* similarity,
                                        float* homography, int B, int NS, int C, int D, int H, int W, void* stream) {
  DINER_CHECK_ARG(ref_cl && src_cl && proj && depth && similarity && homography, "mvs_similarity: null pointer");
  DINER_MVS_LIMITS("mvs_similarity");
  DINER_CHECK_ARG(((uintptr_t)ref_cl | (uintptr_t)src_cl) % 16 == 0, "mvs_similarity: the feature maps must be 16-byte aligned");
  MvsSimArgs a;
  a.ref_cl = ref_cl; a.src_cl = src_cl; a.hom = homography; a.depth = depth; a.sim = similarity;
  a.B = B; a.NS = NS; a.D = D; a.H = H; a.W = W;
  a.PB = pixels_per_block(D);
  a.blocks_per_sample = (H * W + a.PB - 1) / a.PB;
  const long long grid = (long long)a.blocks_per_sample * B;
  DINER_CHECK_ARG(grid < (1ll << 31), "mvs_similarity: %lld workgroups", grid);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mvs_homography, dim3((B * NS + 63) / 64), dim3(64), 0, st, proj, homography, B, NS);
  DINER_LAUNCH_OK();
  DINER_MVS_DISPATCH(launch_similarity, a, (int)grid, st)
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_mvs_similarity_grad_f32(const float* ref_cl, const float* src_cl, const float* homography, const float* depth,
                                             const float* grad_views, const float* grad_aggregated, const float* view_weights, float* d_ref,
                                             float* d_src, int B, int NS, int C, int D, int H, int W, void* stream) {
  DINER_CHECK_ARG(ref_cl && src_cl && homography && depth && d_ref && d_src, "mvs_similarity_grad: null pointer");
  DINER_CHECK_ARG((grad_views != nullptr) != (grad_aggregated != nullptr),
                  "mvs_similarity_grad: give either the per-view gradient or the aggregated one, not both and not neither");
  DINER_CHECK_ARG((grad_aggregated != nullptr) == (view_weights != nullptr),
                  "mvs_similarity_grad: the view weights belong to the aggregated gradient, and it needs them");
  DINER_MVS_LIMITS("mvs_similarity_grad");
  DINER_CHECK_ARG(((uintptr_t)ref_cl | (uintptr_t)src_cl | (uintptr_t)d_ref | (uintptr_t)d_src) % 16 == 0,
                  "mvs_similarity_grad: the feature maps and their gradients must be 16-byte aligned");
  MvsGradArgs a;
  a.ref_cl = ref_cl; a.src_cl = src_cl; a.hom = homography; a.depth = depth; a.g_views = grad_views; a.g_agg = grad_aggregated;
  a.vw = view_weights; a.d_ref = d_ref; a.d_src = d_src;
  a.B = B; a.NS = NS; a.D = D; a.H = H; a.W = W;
  a.PB = pixels_per_block(D);
  a.blocks_per_sample = (H * W + a.PB - 1) / a.PB;
  const long long grid = (long long)a.blocks_per_sample * B;
  DINER_CHECK_ARG(grid < (1ll << 31), "mvs_similarity_grad: %lld workgroups", grid);
  hipStream_t st = (hipStream_t)stream;
  DINER_HIP_OK(hipMemsetAsync(d_src, 0, (size_t)NS * B * H * W * C * sizeof(float), st));
  DINER_MVS_DISPATCH(launch_similarity_grad, a, (int)grid, st)
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_mvs_select_depth_f32(const float* cost, const float* prob_init, const float* hypotheses, float* depth, float* confidence,
                                          float* prob_volume, int B, int D, int H, int W, void* stream) {
  DINER_CHECK_ARG(cost && hypotheses && depth && confidence, "mvs_select_depth: null pointer");
  DINER_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && D >= 1, "mvs_select_depth: B = %d, D = %d, H = %d, W = %d must be >= 1", B, D, H, W);
  DINER_CHECK_ARG((long long)B * D * H * W < (1ll << 31), "mvs_select_depth: B D H W = %lld must stay below 2^31", (long long)B * D * H * W);
  const int total = B * H * W;
  hipLaunchKernelGGL(k_mvs_select_depth, dim3((total + kMvsThreads - 1) / kMvsThreads), dim3(kMvsThreads), 0, (hipStream_t)stream, cost, prob_init,
                     hypotheses, depth, confidence, prob_volume, total, D, H * W);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_mvs_hypotheses_f32(const float* cur_depth, float* hypotheses, int B, int h, int w, int H, int W, int scale, int D,
                                        float half_range, void* stream) {
  DINER_CHECK_ARG(cur_depth && hypotheses, "mvs_hypotheses: null pointer");
  DINER_CHECK_ARG(B >= 1 && h >= 1 && w >= 1, "mvs_hypotheses: B = %d, h = %d, w = %d must be >= 1", B, h, w);
  DINER_CHECK_ARG(scale == 1 || scale == 2 || scale == 4, "mvs_hypotheses: stage scale %d (1, 2 or 4)", scale);
  DINER_CHECK_ARG(H >= scale && W >= scale, "mvs_hypotheses: image %d x %d smaller than the stage scale %d", H, W, scale);
  DINER_CHECK_ARG(D >= 2 && D <= kMvsMaxD, "mvs_hypotheses: D = %d outside [2, %d]", D, kMvsMaxD);
  const int Ho = H / scale, Wo = W / scale;
  DINER_CHECK_ARG((long long)B * D * Ho * Wo < (1ll << 31) && (long long)h * w < (1ll << 31) && (long long)B * h * w < (1ll << 40),
                  "mvs_hypotheses: B D (H / s) (W / s) must stay below 2^31");
  const int total = B * Ho * Wo;
  hipLaunchKernelGGL(k_mvs_hypotheses, dim3((total + kMvsThreads - 1) / kMvsThreads), dim3(kMvsThreads), 0, (hipStream_t)stream, cur_depth,
                     hypotheses, total, h, w, H, W, Ho, Wo, D, half_range);
  DINER_LAUNCH_OK();
  return 0;
}
