// The optimiser step on the device: torch.optim.Adam / AdamW (torch/optim/adam.py, single-tensor, non-capturable route) over ALL parameter
// tensors of a model in one launch -- the reference's `torch.optim.Adam(self.nerf.parameters(), lr=self.lr)` (src/models/diner.py:332-334)
//   optim_table_*        host only: the chunk table, <= DINER_OPTIM_CHUNK elements of one tensor per chunk, one workgroup per chunk
//   k_grad_stats         per chunk: sum g^2 (double) and the number of non-finite g            -> the chunk's partial slot
//   k_grad_stats_final   one workgroup: the partial slots in a fixed order                     -> the state block
//   k_adam               per chunk: the update, with the clip factor / the skip decision read from the state block
//
// Arithmetic: every per-element operation is one fp32 operation rounded where torch's elementwise kernels round (the build's
// -ffp-contract=off; the one fused multiply-add is written out); the two bias corrections are double, from the step count of the state
// block.  No atomics, no workgroup waits for another: the sums of k_grad_stats run per thread in index order, then over the lanes and the
// waves in a fixed tree, then over the chunks in table order, so their bits are a function of the table and the values alone.
//
// The step count lives on the device in two slots: every workgroup of k_adam reads slot `slot` while workgroup 0 writes slot `slot ^ 1`, so no
// workgroup that starts late can see the count this launch wrote.  The caller flips `slot` after every diner_adam_step_f32.
#include "common.hpp"

namespace diner {

namespace {

constexpr int kOptThreads = 256;
constexpr int kOptWaves = kOptThreads / 64;
static_assert(DINER_OPTIM_CHUNK % 4 == 0, "interior chunk boundaries must fall on 16 bytes");
static_assert(sizeof(DinerOptimChunk) == 48 && sizeof(DinerOptimState) == 64, "layouts published in include/diner_hip.h");

struct Partial {          // one per chunk, behind the chunk records
  double sumsq;
  long long nonfinite;
};

struct AdamArgs {
  float b2, w1, w2;       // beta2, 1 - beta1, 1 - beta2: the scalars torch hands its fp32 kernels
  float eps, wd, decay;   // eps, weight_decay (coupled), 1 - lr * weight_decay (decoupled)
  double lr, beta1, beta2, max_norm;
  unsigned flags;
  int slot;
};

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

__device__ __forceinline__ void stat_elem(float g, double& s, long long& bad) {
  s += (double)g * (double)g;                     // a non-finite g makes the norm non-finite, as torch's clip_grad_norm_ reports it
  bad += (__builtin_isfinite(g) ? 0 : 1);
}

__global__ void __launch_bounds__(kOptThreads) k_grad_stats(const DinerOptimChunk* __restrict__ table, Partial* __restrict__ part) {
  __shared__ double red[kOptWaves];
  const DinerOptimChunk ch = table[blockIdx.x];
  const int t = threadIdx.x;
  const float* g = ch.grad;
  double s = 0.0;
  long long bad = 0;
  if (aligned16(g)) {
    const int nvec = ch.numel >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (int i = t; i < nvec; i += kOptThreads) {
      const float4 v = g4[i];
      stat_elem(v.x, s, bad);
      stat_elem(v.y, s, bad);
      stat_elem(v.z, s, bad);
      stat_elem(v.w, s, bad);
    }
    const int i = (nvec << 2) + t;                // the tail: numel % 4 elements
    if (i < ch.numel) stat_elem(g[i], s, bad);
  } else {
    for (int i = t; i < ch.numel; i += kOptThreads) stat_elem(g[i], s, bad);
  }
  s = block_sum_d<kOptWaves>(s, red);
  const double b = block_sum_d<kOptWaves>((double)bad, red);   // <= DINER_OPTIM_CHUNK: exact
  if (t == 0) {
    part[blockIdx.x].sumsq = s;
    part[blockIdx.x].nonfinite = (long long)b;
  }
}

__global__ void __launch_bounds__(kOptThreads) k_grad_stats_final(const Partial* __restrict__ part, int n_chunks, DinerOptimState* __restrict__ st) {
  __shared__ double red[kOptWaves];
  double s = 0.0, b = 0.0;                        // counts stay exact in double below 2^53 elements
  for (int k = threadIdx.x; k < n_chunks; k += kOptThreads) {
    s += part[k].sumsq;
    b += (double)part[k].nonfinite;
  }
  s = block_sum_d<kOptWaves>(s, red);
  b = block_sum_d<kOptWaves>(b, red);
  if (threadIdx.x == 0) {
    st->grad_norm_sq = s;
    st->nonfinite = (long long)b;
  }
}

struct StepScalars {
  float step_size, bc2_sqrt, clip;
};

// torch/optim/adam.py _single_tensor_adam, one element.  g has been read; p, m, v are updated in registers.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamArgs& a, const StepScalars& k) {
  g = __fmul_rn(g, k.clip);                                                     // clip_grad_norm_: g.mul_(coef); coef = 1 without CLIP
  if (a.flags & DINER_ADAM_DECOUPLED_WD) p = __fmul_rn(p, a.decay);             // param.mul_(1 - lr * weight_decay)
  else if (a.wd != 0.0f) g = __fmaf_rn(a.wd, p, g);                            // grad.add(param, alpha=weight_decay)
  m = __fadd_rn(m, __fmul_rn(a.w1, __fsub_rn(g, m)));                           // exp_avg.lerp_(grad, 1 - beta1), weight < 0.5
  v = __fadd_rn(__fmul_rn(v, a.b2), __fmul_rn(__fmul_rn(a.w2, g), g));          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), k.bc2_sqrt), a.eps);   // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  p = __fsub_rn(p, __fmul_rn(k.step_size, __fdiv_rn(m, denom)));                // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ void __launch_bounds__(kOptThreads) k_adam(const DinerOptimChunk* __restrict__ table, DinerOptimState* __restrict__ st, AdamArgs a) {
  __shared__ StepScalars ks;
  __shared__ int skip_s;
  const DinerOptimChunk ch = table[blockIdx.x];
  const int t = threadIdx.x;
  if (t == 0) {
    const long long t_prev = st->step[a.slot], skipped_prev = st->skipped[a.slot];
    const bool skip = (a.flags & DINER_ADAM_SKIP_NONFINITE) && st->nonfinite != 0;
    double clip = 1.0;
    if (a.flags & DINER_ADAM_CLIP) {
      const double coef = a.max_norm / (sqrt(st->grad_norm_sq) + 1e-6);
      clip = coef > 1.0 ? 1.0 : coef;             // a NaN norm stays NaN, as torch.clamp(coef, max=1.0) keeps it
    }
    const double tn = (double)(t_prev + 1);
    const double bc1 = 1.0 - pow(a.beta1, tn), bc2 = 1.0 - pow(a.beta2, tn);
    ks.step_size = (float)(a.lr / bc1);
    ks.bc2_sqrt = (float)sqrt(bc2);
    ks.clip = (float)clip;
    skip_s = skip ? 1 : 0;
    if (blockIdx.x == 0) {                        // the other slot: no workgroup of this launch reads it
      st->step[a.slot ^ 1] = skip ? t_prev : t_prev + 1;
      st->skipped[a.slot ^ 1] = skipped_prev + (skip ? 1 : 0);
      st->clip = skip ? 0.0 : clip;
    }
  }
  __syncthreads();
  const bool skip = skip_s != 0, zero = (a.flags & DINER_ADAM_ZERO_GRADS) != 0;
  if (skip && !zero) return;
  const StepScalars k = ks;
  float *p = ch.param, *g = ch.grad, *m = ch.exp_avg, *v = ch.exp_avg_sq;
  const int n = ch.numel;
  const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
  const int nvec = vec ? n >> 2 : 0;
  float4 *p4 = reinterpret_cast<float4*>(p), *g4 = reinterpret_cast<float4*>(g), *m4 = reinterpret_cast<float4*>(m),
         *v4 = reinterpret_cast<float4*>(v);
  const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (skip) {                                     // nothing is written but the zeroed gradients
    for (int i = t; i < nvec; i += kOptThreads) g4[i] = zero4;
    for (int i = (nvec << 2) + t; i < n; i += kOptThreads) g[i] = 0.0f;
    return;
  }
  for (int i = t; i < nvec; i += kOptThreads) {
    float4 pv = p4[i], mv = m4[i], vv = v4[i];
    const float4 gv = g4[i];
    adam_elem(pv.x, gv.x, mv.x, vv.x, a, k);
    adam_elem(pv.y, gv.y, mv.y, vv.y, a, k);
    adam_elem(pv.z, gv.z, mv.z, vv.z, a, k);
    adam_elem(pv.w, gv.w, mv.w, vv.w, a, k);
    p4[i] = pv;
    m4[i] = mv;
    v4[i] = vv;
    if (zero) g4[i] = zero4;
  }
  for (int i = (nvec << 2) + t; i < n; i += kOptThreads) {      // numel % 4 elements, or the whole chunk where a base pointer is off 16 bytes
    float pv = p[i], mv = m[i], vv = v[i];
    adam_elem(pv, g[i], mv, vv, a, k);
    p[i] = pv;
    m[i] = mv;
    v[i] = vv;
    if (zero) g[i] = 0.0f;
  }
}

// chunks of the n records; < 0 for a bad argument (message set)
long long optim_plan(const DinerOptimTensor* t, int n, const char* who) {
  if (!t || n <= 0) {
    set_error("%s: need n >= 1 tensor records, got n = %d%s", who, n, t ? "" : " and a null record array");
    return -1;
  }
  long long chunks = 0;
  for (int i = 0; i < n; ++i) {
    if (t[i].numel < 0) {
      set_error("%s: record %d has numel = %lld", who, i, t[i].numel);
      return -1;
    }
    if (t[i].numel == 0) continue;
    if (!t[i].param || !t[i].grad || !t[i].exp_avg || !t[i].exp_avg_sq) {
      set_error("%s: record %d (numel %lld) has a null pointer", who, i, t[i].numel);
      return -1;
    }
    chunks += (t[i].numel + DINER_OPTIM_CHUNK - 1) / DINER_OPTIM_CHUNK;
    if (chunks > 0x7fffffffLL) {
      set_error("%s: more than 2^31 - 1 chunks", who);
      return -1;
    }
  }
  return chunks;
}

}  // namespace

}  // namespace diner

using namespace diner;

extern "C" size_t diner_optim_table_bytes(const DinerOptimTensor* t, int n) {
  const long long chunks = optim_plan(t, n, "optim_table_bytes");
  return chunks < 0 ? 0 : (size_t)chunks * (sizeof(DinerOptimChunk) + sizeof(Partial));
}

extern "C" int diner_optim_table_build(const DinerOptimTensor* t, int n, void* host_out, size_t bytes, int* n_chunks) {
  const long long chunks = optim_plan(t, n, "optim_table_build");
  if (chunks < 0) return DINER_E_INVALID;
  DINER_CHECK_ARG(n_chunks, "optim_table_build: null n_chunks");
  const size_t need = (size_t)chunks * (sizeof(DinerOptimChunk) + sizeof(Partial));
  DINER_CHECK_ARG(host_out || need == 0, "optim_table_build: null output buffer");
  DINER_CHECK_ARG(bytes >= need, "optim_table_build: the buffer holds %zu bytes, the table needs %zu", bytes, need);
  DinerOptimChunk* out = (DinerOptimChunk*)host_out;
  long long c = 0;
  for (int i = 0; i < n; ++i)
    for (long long off = 0; off < t[i].numel; off += DINER_OPTIM_CHUNK, ++c) {
      const long long left = t[i].numel - off;
      out[c].param = t[i].param + off;
      out[c].grad = t[i].grad + off;
      out[c].exp_avg = t[i].exp_avg + off;
      out[c].exp_avg_sq = t[i].exp_avg_sq + off;
      out[c].numel = (int32_t)(left < DINER_OPTIM_CHUNK ? left : DINER_OPTIM_CHUNK);
      out[c].tensor = i;
      out[c].offset = off;
    }
  if (need) memset((char*)host_out + (size_t)chunks * sizeof(DinerOptimChunk), 0, (size_t)chunks * sizeof(Partial));
  *n_chunks = (int)chunks;
  return 0;
}

extern "C" int diner_optim_grad_stats(void* table, int n_chunks, DinerOptimState* state, void* stream) {
  DINER_CHECK_ARG(table && state, "optim_grad_stats: null pointer argument");
  DINER_CHECK_ARG(n_chunks >= 1, "optim_grad_stats: n_chunks = %d, need >= 1", n_chunks);
  Partial* part = (Partial*)((char*)table + (size_t)n_chunks * sizeof(DinerOptimChunk));
  hipLaunchKernelGGL(k_grad_stats, dim3(n_chunks), dim3(kOptThreads), 0, (hipStream_t)stream, (const DinerOptimChunk*)table, part);
  DINER_LAUNCH_OK();
  hipLaunchKernelGGL(k_grad_stats_final, dim3(1), dim3(kOptThreads), 0, (hipStream_t)stream, (const Partial*)part, n_chunks, state);
  DINER_LAUNCH_OK();
  return 0;
}

extern "C" int diner_adam_step_f32(const void* table, int n_chunks, DinerOptimState* state, const DinerAdamHyper* h, void* stream) {
  DINER_CHECK_ARG(table && state && h, "adam_step: null pointer argument");
  DINER_CHECK_ARG(n_chunks >= 1, "adam_step: n_chunks = %d, need >= 1", n_chunks);
  DINER_CHECK_ARG(h->slot == 0 || h->slot == 1, "adam_step: slot = %d, need 0 or 1", h->slot);
  DINER_CHECK_ARG((h->flags & ~(unsigned)DINER_ADAM_ALL_FLAGS) == 0, "adam_step: unknown flag bits 0x%x", h->flags);
  DINER_CHECK_ARG(h->lr >= 0.0 && h->eps >= 0.0 && h->weight_decay >= 0.0, "adam_step: lr = %g, eps = %g, weight_decay = %g must be >= 0",
                  h->lr, h->eps, h->weight_decay);
  DINER_CHECK_ARG(h->beta1 >= 0.0 && h->beta1 < 1.0 && h->beta2 >= 0.0 && h->beta2 < 1.0, "adam_step: betas (%g, %g) must lie in [0, 1)",
                  h->beta1, h->beta2);
  DINER_CHECK_ARG(!(h->flags & DINER_ADAM_CLIP) || h->max_norm > 0.0, "adam_step: CLIP needs max_norm > 0, got %g", h->max_norm);
  AdamArgs a;
  a.max_norm = h->max_norm;
  a.b2 = (float)h->beta2;
  a.w1 = (float)(1.0 - h->beta1);
  a.w2 = (float)(1.0 - h->beta2);
  a.eps = (float)h->eps;
  a.wd = (float)h->weight_decay;
  a.decay = (float)(1.0 - h->lr * h->weight_decay);
  a.lr = h->lr;
  a.beta1 = h->beta1;
  a.beta2 = h->beta2;
  a.flags = h->flags;
  a.slot = h->slot;
  hipLaunchKernelGGL(k_adam, dim3(n_chunks), dim3(kOptThreads), 0, (hipStream_t)stream, (const DinerOptimChunk*)table, state, a);
  DINER_LAUNCH_OK();
  return 0;
}
