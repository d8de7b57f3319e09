/*
 * diner_hip.h -- C ABI of libdiner_hip.so: DINER's volumetric-rendering hot path on MI355X (gfx950).
 *
 * The reference (malteprinzler/diner) is pure Python/PyTorch and has no FFI of its own; the
 * boundary it offers is the Python module API of the src/models Python modules.  Each entry point below replaces
 * the body of one of those Python functions (cited as file:line in /root/reference) and is what a
 * maintainer would bind with ctypes from those modules -- see INTEGRATION.md.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HIP) to contiguous row-major fp32 unless stated;
 *   - every call only ENQUEUES work on the caller's stream (hipStream_t passed as void*);
 *     no hidden synchronisation, no global mutable state besides the thread-local error string, and no
 *     device allocation -- with one exception: diner_mlp_create() hipMallocs the buffers of the packed-weights
 *     handle it returns (freed by diner_mlp_destroy) and synchronises `stream` once before it returns;
 *   - return value: 0 = ok, negative = DINER_E_*; diner_last_error() gives the message;
 *   - the caller (PyTorch's caching allocator in the Python host) owns all buffers; the library
 *     owns only the packed-weights handle created by diner_mlp_create().
 */
#ifndef DINER_HIP_H
#define DINER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DINER_ABI_VERSION 6   /* the *_long_f32 entry points were added without a bump: new symbols, no v6 contract changed */

/* Source views a scene may have (DinerScene.nv).  The fused field / training kernels are built for exactly 4 (every shipped config);
 * the sampler, diner_index_f32, the generic path (diner_field_inputs_generic_*) and the *_views_f32 field entries (the fused kernels over
 * groups of four views) take 1 .. DINER_MAX_VIEWS.  Added without an ABI bump: no struct or signature changed. */
#define DINER_MAX_VIEWS 16

#define DINER_E_INVALID     (-1)  /* bad argument (null pointer, size, unsupported configuration) */
#define DINER_E_UNSUPPORTED (-2)  /* configuration outside what the kernels are built for        */
#define DINER_E_HIP         (-3)  /* a HIP runtime call failed                                     */

/* Per-object scene state: what the reference keeps on PixelNeRF / SpatialEncoder after encode()
 * (pixelnerf.py:47-51; image_encoder.py:232-236, :290-291). */
typedef struct DinerScene {
  const float* latent_cl;   /* (NV, Hf, Wf, C)  feature map, CHANNELS-LAST (re-laid-out once per encode) */
  const float* latent_proj; /* (3, NV, Hf, Wf, C) lin_z[b](latent)+bias, written by diner_scene_prepare_f32; the field
                               entry points gather from these maps (resnetfc.py:153-155 hoisted out of the sample loop).
                               Maps 1 and 2 also carry the fc_1 bias of the block before them (the two constants are added to
                               the residual stream at the same point): opaque to the caller, valid for the MLP handle that
                               prepared them */
  const float* depth;       /* (NV, Hs, Ws)     source depth maps, 0 = background                          */
  const float* depth_std;   /* (NV, Hs, Ws)     depth standard deviation                                    */
  const float* normals;     /* (NV, 3, Hs, Ws)  normal maps (planar, as produced by depth2normal)          */
  /* ---- the only HOST pointers of this struct (suffix _host): three tiny camera arrays, read on the host at call time and
   *      copied by value into the kernel arguments (SGPRs); never dereferenced on the device ---- */
  const float* poses_host;  /* HOST (NV, 4, 4)  world->camera extrinsics, row-major (pixelnerf.py:47)               */
  const float* focal_host;  /* HOST (NV, 2)     fx, fy                               (pixelnerf.py:49)               */
  const float* c_host;      /* HOST (NV, 2)     cx, cy                               (pixelnerf.py:48)               */
  const float* std_pad_scale; /* (100)          multipliers exp(e/12*ln2), e = 0..99, of the exponential std padding
                                                 (torch_helpers.py:110-120 with pad_size=100, pad_double_width=12,
                                                 image_encoder.py:185-194); computed by the host exactly as the
                                                 reference does so that padded sigma values are bit-identical        */
  float img_w, img_h;       /* PixelNeRF.image_shape = [W, H] (pixelnerf.py:50-51)                         */
  float feature_padding;    /* SpatialEncoder.feature_padding (image_encoder.py:59), 32 in the shipped configs */
  int32_t nv, C, Hf, Wf, Hs, Ws; /* nv: source views, 1 .. DINER_MAX_VIEWS.  Entries built for the fused kernels (field, scene preparation,
                               shipped-shape training, diner_train_inputs_f32) return DINER_E_UNSUPPORTED for 5 .. 16 views (the
                               *_views_f32 field entries take them); every entry returns DINER_E_INVALID outside [1, DINER_MAX_VIEWS] */
  uint64_t proj_stamp;      /* diner_mlp_stamp() of the handle that wrote latent_proj (set by the caller after
                               diner_scene_prepare_f32).  The field entry points return DINER_E_INVALID when it is not the
                               stamp of the handle they are called with: maps prepared with another (or an older) handle carry
                               that handle's biases */
  const void* latent_proj_f16; /* ABI v4: the same three maps as fp16 (3, NV, Hf, Wf, C), channels in the order the plain-fp16 field
                               kernel consumes them, written by diner_scene_prepare_f16 from latent_proj (same proj_stamp).  Only
                               DINER_PRECISION_F16 reads it (half the gather bytes of that mode); NULL for the other modes */
  uint64_t proj_stamp_f16;  /* ABI v5: diner_mlp_stamp() of the handle whose latent_proj the fp16 copy was made from (set by the caller after
                               diner_scene_prepare_f16).  DINER_PRECISION_F16 returns DINER_E_INVALID when it is not the stamp of the handle
                               it is called with: a caller that re-ran diner_scene_prepare_f32 with new weights but not _prepare_f16 would
                               otherwise render from stale fp16 maps without an error */
} DinerScene;

/* ResnetFC parameters as the reference stores them (nn.Linear: weight (out,in), bias (out));
 * resnetfc.py:72-127.  Host or device pointers are both accepted by diner_mlp_create (flag). */
typedef struct DinerMlpParams {
  int32_t d_in, d_latent, d_hidden, d_out, n_blocks, combine_layer;
  /* positional encoding that produces the d_in inputs (pixelnerf.py:15-18, positional_encoding.py:12-31): the field
   * entry points encode x_c (3 -> 3*(2F+1)) and the depth difference (1 -> 2F+1) in registers.  num_freqs must be 6
   * and include_input non-zero (d_in = 55); freq_factor is honoured (6.28 in every shipped config). */
  int32_t num_freqs, include_input;
  float freq_factor;
  const float* lin_in_w;  const float* lin_in_b;       /* (d_hidden, d_in), (d_hidden)          */
  const float* lin_out_w; const float* lin_out_b;      /* (d_out, d_hidden), (d_out)            */
  const float* const* fc0_w; const float* const* fc0_b; /* n_blocks x (d_hidden,d_hidden),(d_hidden) */
  const float* const* fc1_w; const float* const* fc1_b;
  const float* const* lin_z_w; const float* const* lin_z_b; /* min(combine_layer,n_blocks) x (d_hidden,d_latent) */
} DinerMlpParams;

typedef struct DinerMlp DinerMlp;   /* opaque: weights re-packed into MFMA-fragment order, resident in HBM */

int         diner_abi_version(void);
const char* diner_last_error(void);

/* ---- packed weights ---------------------------------------------------------------------------
 * Packs the ResnetFC parameters (DEVICE pointers) into stage-tile order on `stream`.
 * Supported: d_in=55, d_latent=512, d_hidden=512, d_out=4, n_blocks=5, combine_layer=3, num_freqs=6, include_input=1
 * (the configuration of configs/train_dtu.yaml:39-50 and train_facescape.yaml), NV = 4; anything else returns
 * DINER_E_UNSUPPORTED before any device work.  A failed call leaves no allocation behind. */
int diner_mlp_create(const DinerMlpParams* p, void* stream, DinerMlp** out);
int diner_mlp_destroy(DinerMlp* mlp);
/* ABI v6: new parameter values into an EXISTING handle, packed on `stream` -- no allocation and no synchronisation (diner_mlp_create
 * hipMallocs ~12 buffers, waits for the stream once, and diner_mlp_destroy hipFrees them: three device-wide synchronisations per optimiser
 * step when a training loop re-creates its handle; resnetfc.py:72-127 under the optimiser's in-place updates, diner.py:217-290).  The
 * parameter tensors must stay valid until the packing has run on `stream`.  The handle gets a new diner_mlp_stamp(): maps projected with
 * the old values are refused.  The weight range is not read back: diner_mlp_weights_fit_f16x3 and the inference entry points read it
 * (one stream wait) the first time they need it after an update; the fused training forward never does -- it tests the range on the device.
 * flags: DINER_MLP_UPDATE_TRAIN_ONLY packs only what diner_field_train_forward_fused_f32 / _batch_f32 read (the four-wave f16x3 layouts,
 * biases, the constants of the projected maps): the inference entry points then return DINER_E_INVALID for this handle until an update
 * without the flag. */
#define DINER_MLP_UPDATE_TRAIN_ONLY 1
int diner_mlp_update(DinerMlp* mlp, const DinerMlpParams* p, int flags, void* stream);
/* Largest |weight| over all weight matrices (biases stay fp32 in every mode), reduced on the device at pack time (one 4-byte read back, after a
 * stream synchronise): DINER_PRECISION_F16X3 / _F16 carry the weights x16 as fp16 and need it below 1024.
 * Returns 1 when the f16 modes may be used with this handle, 0 when not, <0 on error; *max_abs (optional) receives the value. */
int diner_mlp_weights_fit_f16x3(const DinerMlp* mlp, float* max_abs);
/* Identity of a packed-weights handle: unique per diner_mlp_create call of the process, never 0.  Goes into
 * DinerScene.proj_stamp after diner_scene_prepare_f32(scene, mlp, ...). */
uint64_t diner_mlp_stamp(const DinerMlp* mlp);
/* Number of field launches with this handle whose fp16-operand pass left the fp16 range (or met a non-finite input) and were
 * recomputed by the exact-fp32 kernels on the device (see DINER_PRECISION_* below) -- a 2-3x slower launch that is otherwise
 * invisible.  Waits for `stream` (one 4-byte read back); `reset` != 0 zeroes the counter. */
int diner_mlp_fallback_count(const DinerMlp* mlp, long long* launches, int reset, void* stream);

/* ---- a1+a2+a3+a4: NeRFRendererDGS.sample_depthguided + fill_up_uniform_samples ---------------
 * (nerf_renderer.py:39-63, :65-190, :367-397; torch_helpers.py:215-223; image_encoder.py:148-223)
 *   rays         (NR, 8)  [o(3), d(3), near, far]
 *   t_base       (n_cand) the stratification offsets torch.linspace(0, 1-1/n_cand, n_cand)
 *   noise_*      explicit noise (parity mode) or NULL -> counter-based Philox4x32-10 keyed by (`seed`, ray_index0 + i) for ray i of
 *                the call: ray_index0 = index of rays[0] in the caller's ray list, so that a frame rendered with one seed does not
 *                depend on how its rays are split into batches or sharded across GPUs (the reference's noise depends on both)
 *                noise_coarse (NR,n_cand) U[0,1); noise_gauss (NR,G) N(0,1); noise_fill (NR,K) U[0,1)
 *                indexed by the SORTED column of the empty slot
 *   z_out        (NR, K)  ascending z per ray
 *   z_unfilled   optional (NR, K): the sampler output before the fill (zeros = empty), or NULL
 * Limits: n_cand <= 1024, K <= 256, 0 <= G <= K. */
int diner_sample_depthguided_f32(const DinerScene* scene, const float* rays, int NR, int n_cand, int K, int G,
                                 float depth_diff_max, const float* t_base,
                                 const float* noise_coarse, const float* noise_gauss, const float* noise_fill,
                                 uint64_t seed, long long ray_index0, float* z_out, float* z_unfilled, void* stream);

/* Stage-level entry for tests: fill_up_uniform_samples alone (nerf_renderer.py:367-397).  Limits: K <= 256. */
int diner_fill_uniform_f32(const float* z_in, const float* rays, int NR, int K, const float* noise_fill,
                           uint64_t seed, long long ray_index0, float* z_out, void* stream);

/* Long-ray entries (the reference's --nsamples takes any count, create_prediction_folder.py:43-47): same signatures and
 * arguments as the bounded siblings above / below, whole range, the kernel picked from the sizes.
 * Limits: 1 <= K <= 1024, 1 <= n_cand <= 4096, 0 <= G <= K; anything outside is DINER_E_INVALID before any device work.
 * Where the bounded kernels fit (K <= 256 and n_cand <= 1024) they run with the same arguments, so results there are
 * bit-identical to diner_sample_depthguided_f32 / diner_fill_uniform_f32 / diner_composite_f32.  Above, the sampler runs one
 * workgroup per ray (same per-candidate likelihood, pick rule and noise keys: a ray's picks and draws do not depend on the
 * kernel, nor on batching) and the compositor carries 16 samples per lane.  K > n_cand keeps K columns, the extra slots
 * filled stratified (the reference returns min(K, n_cand) columns). */
int diner_sample_depthguided_long_f32(const DinerScene* scene, const float* rays, int NR, int n_cand, int K, int G,
                                      float depth_diff_max, const float* t_base,
                                      const float* noise_coarse, const float* noise_gauss, const float* noise_fill,
                                      uint64_t seed, long long ray_index0, float* z_out, float* z_unfilled, void* stream);
int diner_fill_uniform_long_f32(const float* z_in, const float* rays, int NR, int K, const float* noise_fill,
                                uint64_t seed, long long ray_index0, float* z_out, void* stream);

/* The sampler with what it knows about the ray beside the samples: the arguments, checks, error codes, limits and z_out (bit for
 * bit, explicit or Philox noise) of diner_sample_depthguided_f32 / _long_f32, with z_unfilled replaced by four optional outputs,
 * each written only where its pointer is not NULL:
 *   z_ordered  (NR, K)      the sampler output before the fill in the reference's slot order (nerf_renderer.py:172-190): the
 *                           K - G picks by descending surface likelihood -- equal likelihood bits: lower candidate index first,
 *                           the rule of the ties at the cut-off --, empty pick slots (z = 0) after them, then the G gaussian samples
 *   slot_L     (NR, K - G)  likelihood of the pick in each slot (0 = empty)
 *   slot_idx   (NR, K - G)  int32: index of its candidate among the ray's n_cand (-1 = empty)
 *   stats      (NR, 4)      sum of the candidates' likelihoods L, sum of O = L_i * prod_{j<i}(1 - L_j) -- the depth maps' probability
 *                           1 - prod(1 - L) that the ray meets a surface --, and the O-weighted mean and standard deviation of the
 *                           candidate depths (the gaussian the G samples are drawn from, :183); all 0 where the ray sees no surface
 * K - G = 0 is legal: slot_L / slot_idx are not touched.  The long entry runs the bounded info kernel where it fits
 * (K <= 256 and n_cand <= 1024): results there equal the bounded entry's bit for bit. */
int diner_sample_depthguided_info_f32(const DinerScene* scene, const float* rays, int NR, int n_cand, int K, int G,
                                      float depth_diff_max, const float* t_base,
                                      const float* noise_coarse, const float* noise_gauss, const float* noise_fill,
                                      uint64_t seed, long long ray_index0, float* z_out,
                                      float* z_ordered, float* slot_L, int32_t* slot_idx, float* stats, void* stream);
int diner_sample_depthguided_info_long_f32(const DinerScene* scene, const float* rays, int NR, int n_cand, int K, int G,
                                           float depth_diff_max, const float* t_base,
                                           const float* noise_coarse, const float* noise_gauss, const float* noise_fill,
                                           uint64_t seed, long long ray_index0, float* z_out,
                                           float* z_ordered, float* slot_L, int32_t* slot_idx, float* stats, void* stream);
int diner_composite_long_f32(const float* field, const float* z, const float* rays, int NR, int K, int white_bkgd,
                             float* rgb_out, float* depth_out, float* weights_out, void* stream);

/* ---- per-scene preparation: hoist of the three lin_z projections (resnetfc.py:153-155) ---------
 * lin_z[b] is linear and bilinear/border weights sum to 1, so lin_z[b](interp(latent)) == interp(lin_z[b](latent)):
 * the projections are applied once per feature-map pixel here instead of once per (sample, view).  Must be called
 * (and scene->latent_proj set to the output buffer of diner_scene_proj_bytes(scene) bytes) whenever the latent map or
 * the lin_z parameters change, before any diner_field_* / diner_render_f32 call on that scene. */
size_t diner_scene_proj_bytes(const DinerScene* scene);
int diner_scene_prepare_f32(const DinerScene* scene, const DinerMlp* mlp, float* latent_proj_out, void* stream);
/* ABI v4, DINER_PRECISION_F16 only ("fp16 MLP on MFMA", create_prediction_folder.py:44-47 with configs/evaluate_diner_on_facescape.yaml):
 * fp16 copy of scene->latent_proj (which must be set and current) into latent_proj_f16_out, diner_scene_proj_f16_bytes(scene) bytes;
 * the caller then stores the pointer in scene->latent_proj_f16.  Values beyond the fp16 range become inf and end up in the launch's
 * overflow flag (the gated exact-fp32 pass recomputes it from latent_proj). */
size_t diner_scene_proj_f16_bytes(const DinerScene* scene);
int diner_scene_prepare_f16(const DinerScene* scene, void* latent_proj_f16_out, void* stream);

/* ---- arithmetic of the MLP GEMMs: a PER-CALL argument of the field entry points (no process-wide state) ---------
 * DINER_PRECISION_FP32  exact fp32 MFMA (v_mfma_f32_16x16x4_f32), an fmaf chain per output (mlp.hip).
 * DINER_PRECISION_F16X3 "f16x3" split products: each fp32 product a*w is evaluated as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi
 *                       on the fp16 MFMA with fp32 accumulation and power-of-two pre-scaling; ~2^-21 relative error per
 *                       product, end-to-end results within fp32 round-off class of the reference (parity tests hold it
 *                       to the same 1e-4 bar as FP32).  Feature-sliced kernels (mlp_h3n.hip).  Requires |w| < 1024 and
 *                       hidden activations < 6.5e4 (weights are checked by the host; see diner_mlp_weights_fit_f16x3);
 *                       one projected map (NV*Hf*Wf*2 KB) must stay below 4 GiB, else DINER_E_UNSUPPORTED.
 * DINER_PRECISION_F16   plain fp16 operands (hi parts only, one MFMA per product), fp32 accumulation, same kernels:
 *                       BASELINE configs[4] ("fp16 MLP on MFMA").  ~1e-3 relative on rendered colours: OUTSIDE the
 *                       1e-4 parity bar, never a default.
 * diner_mlp_forward_f32 (explicit matrices), diner_scene_prepare_f32 and the training path always use exact fp32. */
#define DINER_PRECISION_FP32  0
#define DINER_PRECISION_F16X3 1
#define DINER_PRECISION_F16   3   /* (2 is retired: it meant the parity-grade split mode in ABI v1 and is rejected, so that an old
                                     caller passing the bare integer cannot end up in the reduced-precision mode) */

/* ---- a5+a6+a7+a8: PixelNeRF.forward at ray samples -------------------------------------------
 * (pixelnerf.py:55-145; positional_encoding.py:33-53; image_encoder.py:97-170; resnetfc.py:129-159)
 * Points are o + z*d for every (ray, sample); view directions are the ray directions.
 *   precision  DINER_PRECISION_* (above)
 *   field_out  (NR*K, 4) = [sigmoid(r,g,b), relu(sigma)]
 *   workspace  diner_field_workspace_bytes(NR*K) bytes of device scratch: the hand-over between the per-view and the post kernel (the view
 *              mean of the residual stream, 2 KB per point) and the flag block.  DINER_PRECISION_F16X3 hands over a second plane of the same
 *              size (the view mean of relu(h) of the last per-view block, whose fc_1 the post kernel runs once per point); that one lives
 *              in a buffer the library owns per (device, stream), grown when a launch needs more than the stream has had and kept until
 *              diner_field_release_buffers() -- the training forward on the fused kernels uses it too. */
size_t diner_field_workspace_bytes(long long n_points);
/* Frees the library-owned hand-over buffers of every device and stream (waits for the device); the next f16x3 launch allocates its own
 * again.  Returns 0 when there was nothing to free -- no device is touched then.  New symbol, no ABI bump. */
int diner_field_release_buffers(void);
int diner_field_from_rays_f32(const DinerScene* scene, const DinerMlp* mlp, const float* rays, const float* z,
                              int NR, int K, int precision, float* field_out, void* workspace, void* stream);
/* Same, explicit points / view directions (P,3): PixelNeRF.forward(xyz, viewdirs) (pixelnerf.py:55). */
int diner_field_from_points_f32(const DinerScene* scene, const DinerMlp* mlp, const float* xyz, const float* viewdirs,
                                long long P, int precision, float* field_out, void* workspace, void* stream);

/* ---- the same for scenes with ANY number of source views, 1 .. DINER_MAX_VIEWS (pixelnerf.py:67 takes any) -------------------------
 * The mean over the views (resnetfc.py:148-151) is linear: an NV-view scene runs as ceil(NV / 4) launches of the four-view per-view
 * kernel over groups of four cameras, each adding (1 / NV) x the sum over its live views into the same 2 KB-per-point hand-over (f16x3:
 * into both of its planes, see diner_field_workspace_bytes), and one
 * unchanged post kernel.  A partial group's spare columns recompute one of its own views and are left out of the sum.  Arguments,
 * workspace size and results as the four-view namesakes above; NV = 4 IS the four-view entry (same bits).  New symbols, no ABI bump.
 *   diner_scene_proj_views_bytes    3 NV Hf Wf 512 4 bytes for 1 <= NV <= DINER_MAX_VIEWS, else 0
 *   diner_scene_prepare_views_f32   diner_scene_prepare_f32 for any such NV (set scene->latent_proj / proj_stamp as there)
 *   precision                       DINER_PRECISION_F16X3 (gated exact-fp32 repeat over all groups behind it, as above) or _FP32;
 *                                   DINER_PRECISION_F16 with NV != 4 is DINER_E_UNSUPPORTED (the plain-fp16 kernels are four-view)
 *   f16x3 limit                     the 32-bit tap offsets span ONE group's maps: min(NV, 4) Hf Wf 2 KB below 4 GiB, else DINER_E_UNSUPPORTED
 * Validation before any device work: NV outside [1, DINER_MAX_VIEWS] is DINER_E_INVALID; then handle, stamp and configuration. */
size_t diner_scene_proj_views_bytes(const DinerScene* scene);
int diner_scene_prepare_views_f32(const DinerScene* scene, const DinerMlp* mlp, float* latent_proj_out, void* stream);
size_t diner_field_views_workspace_bytes(long long n_points);
int diner_field_from_rays_views_f32(const DinerScene* scene, const DinerMlp* mlp, const float* rays, const float* z,
                                    int NR, int K, int precision, float* field_out, void* workspace, void* stream);
int diner_field_from_points_views_f32(const DinerScene* scene, const DinerMlp* mlp, const float* xyz, const float* viewdirs,
                                      long long P, int precision, float* field_out, void* workspace, void* stream);
int diner_render_views_f32(const DinerScene* scene, const DinerMlp* mlp, const float* rays, const float* z, int NR, int K,
                           int white_bkgd, int precision, float* rgb_out, float* depth_out, float* weights_out,
                           float* field_ws, void* workspace, void* stream);

/* ---- a7 alone: ResnetFC.forward(zx, combine_dim) on an explicit (NV, B, d_latent+d_in) matrix --
 * workspace: diner_mlp_forward_workspace_bytes(B) bytes. */
size_t diner_mlp_forward_workspace_bytes(long long B);
int diner_mlp_forward_f32(const DinerMlp* mlp, const float* zx, long long B, float* out /* (B,4) raw */,
                          void* workspace, void* stream);

/* ---- a9: compositing (nerf_renderer.py:299-301, :341-360) ------------------------------------
 *   field (NR*K,4), z (NR,K), rays (NR,8) -> rgb (NR,3), depth (NR), weights (NR,K) or NULL.  Limits: K <= 256
 *   (diner_composite_long_f32 above: K <= 1024). */
int diner_composite_f32(const float* field, const float* z, const float* rays, int NR, int K, int white_bkgd,
                        float* rgb_out, float* depth_out, float* weights_out, void* stream);

/* a9 with the ray's opacity and depth spread as two more per-ray outputs; new symbol, no ABI bump.  The reference computes the opacity,
 * pix_alpha = weights.sum(-1) (nerf_renderer.py:359), uses it for the white background and never returns it.
 *   alpha_out      (NR) or NULL: sum_k w_k, the value the white background is blended with
 *   depth_var_out  (NR) or NULL: max(0, sum_k w_k (z_k - depth)^2) around the unnormalised depth = sum_k w_k z_k written to depth_out, in the
 *                  centred two-pass form; the sum can be negative only where a weight is (a sample beyond `far`, :301), and reads 0 there.
 *                  An inference diagnostic: it has no adjoint (diner_composite_aux_bwd_f32 takes no gradient for it).
 * rgb, depth and weights are those of diner_composite_long_f32 bit for bit.  Limits: K <= 1024 (4 samples per lane up to 256, 16 above);
 * NULL rgb_out / depth_out or sizes outside are DINER_E_INVALID before any device work. */
int diner_composite_aux_f32(const float* field, const float* z, const float* rays, int NR, int K, int white_bkgd,
                            float* rgb_out, float* depth_out, float* weights_out, float* alpha_out, float* depth_var_out,
                            void* stream);

/* ---- a10: NeRFRendererDGS.composite / forward (nerf_renderer.py:286-365, :399-424) -----------
 * field + composite in one call; `field_ws` is (NR*K,4) scratch the caller provides. */
int diner_render_f32(const DinerScene* scene, const DinerMlp* mlp, const float* rays, const float* z, int NR, int K,
                     int white_bkgd, int precision, float* rgb_out, float* depth_out, float* weights_out,
                     float* field_ws, void* workspace, void* stream);

/* diner_render_f32 / diner_render_views_f32 with the opacity and depth-spread outputs of diner_composite_aux_f32 (pix_alpha of
 * nerf_renderer.py:359; either pointer may be NULL): the same field code as their namesakes, then the aux compositor, hence K <= 1024.
 * The compositor's argument checks (NULL rgb_out / depth_out, NR, K) come first: DINER_E_INVALID before any device work. */
int diner_render_aux_f32(const DinerScene* scene, const DinerMlp* mlp, const float* rays, const float* z, int NR, int K,
                         int white_bkgd, int precision, float* rgb_out, float* depth_out, float* weights_out,
                         float* field_ws, void* workspace, float* alpha_out, float* depth_var_out, void* stream);
int diner_render_views_aux_f32(const DinerScene* scene, const DinerMlp* mlp, const float* rays, const float* z, int NR, int K,
                               int white_bkgd, int precision, float* rgb_out, float* depth_out, float* weights_out,
                               float* field_ws, void* workspace, float* alpha_out, float* depth_var_out, void* stream);

/* ---- stage-level entries that back the reference's small public methods ---------------------- */
/* PositionalEncoding.forward (positional_encoding.py:33-53): x (N,d_in) -> (N, d_in*(2F+include_input)) */
int diner_posenc_f32(const float* x, long long N, int d_in, int num_freqs, float freq_factor, int include_input,
                     float* out, void* stream);
/* SpatialEncoder.index / index_depth / index_depth_std / index_normal (image_encoder.py:97-223):
 *   uv (NV, N, 2) in [-1,1] -> out (NV, Cout, N); mode: 0 latent (bilinear/border, Cout=C),
 *   1 depth (nearest/border), 2 depth_std (nearest on the 100px exponential padding, zeros), 3 normal. */
int diner_index_f32(const DinerScene* scene, int mode, const float* uv, long long N, float* out, void* stream);

/* ---- per-image preparation either side of the renderer ------
 * depth2normal (reference src/util/depth2normal.py:7-87): dmap (N,1,H,W) device, K (N,3,3) device ->
 *   normals (N,3,H,W) device: normalize(cross(down - up, right - left)) of the back-projected pixel centres with
 *   replicate padding; pixels with a background neighbour take the un-cleaned normal of the pixel shifted away from
 *   the hole; 0 where depth == 0 (NaN where the reference produces 0/0). */
int diner_depth2normal_f32(const float* dmap, const float* K, int N, int H, int W, float* normals, void* stream);
/* gen_rays (reference src/util/cam_geometry.py:5-48): rays [ray0, ray0 + n_rays) of the row-major (H, W) pixel-centre
 *   ray list of each of B cameras -> out (B, n_rays, 8) device = [origin(3), world direction(3), near, far].
 *   extrinsics (B,4,4) world->camera, intrinsics (B,3,3), z_near / z_far (B): HOST float32; B <= 16 per call.
 *   A sharded rank passes its own [ray0, ray0 + n_rays) (diner_amd/render.py::shard_range). */
int diner_gen_rays_f32(const float* extrinsics, const float* intrinsics, const float* z_near, const float* z_far, int B,
                       int W, int H, long long ray0, long long n_rays, float* out, void* stream);

/* Image output (row f3): what DINER.create_prediction_folder does with a rendered image before it is written
 * (diner.py:119-133): torchvision.utils.save_image's quantisation, uint8(clamp(v * 255 + 0.5, 0, 255)), of a (3,H,W)
 * image into (H,W,3) bytes; and torch_cmap (torch_helpers.py:42-75): per-image min / max (NaNs skipped; the keys come back
 * as order-preserving int32 images of the floats, see diner_amd/imageio.py), then the matplotlib lookup
 * index = int((x - vmin) / (vmax - vmin) * 256) clipped to [0, 255] in float64 through a 256 x 3 uint8 table that the
 * host quantised the same way. */
int diner_quantize_rgb_u8(const float* img, int H, int W, unsigned char* out, void* stream);
int diner_minmax_f32(const float* x, long long n, float* out2, void* stream);
int diner_colormap_u8(const float* x, long long n, const unsigned char* lut_u8, double vmin, double vmax,
                      unsigned char* out, void* stream);

/* ---- training path: building blocks of the un-fused forward that keeps activations and
 * of the backward pass that torch autograd performs in DINER.calc_losses (diner.py:217-290); driven by
 * diner_amd/train.py.  All pointers are device pointers unless noted; enqueue-only on `stream`.
 *
 * General fp32 GEMM on the matrix cores, C (M x N, row stride ldc) = op(A) (M x K) . op(B) (K x N), row-major:
 *   flags: 1 A is stored K x M, 2 B is stored N x K (torch Linear weights: y = x W^T), 4 / 8 relu applied to A / B while
 *   loading, 16 C += result, 32 atomicAdd into C (required for k_split > 1: weight gradients reduce over ~1e4 rows),
 *   64 exact fp32 MFMA products.  Without flag 64 the product runs as "bf16x6": each fp32 operand is split into three bf16
 *   terms and the six products above 2^-24 are accumulated in fp32 on the bf16 MFMA (2.6x the fp32 MFMA peak; bf16 has fp32's
 *   exponent range, so no scaling and no range limits) -- products as accurate as fp32 rounding itself (ragged and skinny
 *   shapes ride along in zero-padded 128 x 128 x 32 tiles);
 *   bias (N) added to every row, mask (M x N, stride ldc): C = 0 where mask <= 0 (relu adjoint). */
int diner_gemm_f32(const float* A, const float* B, float* C, long long M, int N, int K, int lda, int ldb, int ldc, int flags,
                   const float* bias, const float* mask, int k_split, void* stream);
/* The 512 x 512 layer products of the training path on the feature-sliced kernel (train_lin512.hip, entry point in train_512.hip; what the two calls below use for
 * the forward and data-gradient products of every fc_0 / fc_1 / lin_z layer): Y (M, ldy) [+]= act(X (M, ldx)) op(W) [+ bias] [+ resid],
 * W (512, 512) row-major fp32; transpose = 0: op(W) = W^T (y = x W^T, the nn.Linear forward), 1: op(W) = W (dx = dy W).
 *   flags: 1 relu on X while it is staged, 2 Y += result, 4 (transpose = 0 only) the f16x3 arithmetic of the inference kernels -- two
 *   fp16 planes per operand, three product terms: half the MFMAs, the same accuracy class, |X| < 65504 (the training forward runs its
 *   products this way first and repeats one in bf16x6 when an operand was out of range; this entry does not);
 *   bias (512) / resid (M, ldy) / mask (M, ldy: Y = 0 where mask <= 0) or NULL;
 *   wpack: diner_linear512_pack_bytes() bytes of device scratch (W is packed into three bf16 planes there, then multiplied).
 * Products as accurate as fp32 rounding (six-term split-bf16, no range limits).  ldx, ldy multiples of 4, pointers 16-byte aligned. */
size_t diner_linear512_pack_bytes(void);
int diner_linear512_f32(const float* X, const float* W, float* Y, long long M, int ldx, int ldy, int transpose, int flags,
                        const float* bias, const float* resid, const float* mask, void* wpack, void* stream);
/* The weight / bias gradient of a 512 x 512 layer on the persistent kernel of train_wgrad512.hip (what diner_field_train_backward_f32 uses):
 * dW (512, 512) += dY^T act(X), db (512, or NULL) += column sums of dY, over M >= 1 rows of dY (M, ldy) and X (M, ldx); relu_x != 0 applies
 * relu to X while it is staged.  Both outputs are ACCUMULATED: zero them first.  scratch: NULL (row chunks add into dW with atomics) or
 * diner_wgrad512_scratch_bytes() bytes of device memory (every chunk stores its partial dW there and one pass sums them: what the training
 * step uses; 32 atomics per element cost as much as the products of a 20480-row batch).  ldy even, ldx a multiple of 4, dY 8-byte and
 * X 16-byte aligned.  Six-term split-bf16 products (fp32-class accuracy, no range limits). */
size_t diner_wgrad512_scratch_bytes(void);
int diner_wgrad512_f32(const float* dY, const float* X, float* dW, float* db, long long M, int ldy, int ldx, int relu_x, void* scratch,
                       void* stream);
/* Per-(view, point) MLP inputs of PixelNeRF.forward (pixelnerf.py:91-128) for explicit points xyz / viewdirs (P,3):
 *   feat (NV*P, 64) the 55 encoded inputs zero-padded, tap_row (NV*P, 4) int32 texel rows of the channels-last latent,
 *   tap_w (NV*P, 4) bilinear weights, lat (NV*P, 512) the interpolated latent (SpatialEncoder.index). */
int diner_train_inputs_f32(const DinerScene* scene, const float* xyz, const float* viewdirs, long long P, float freq_factor,
                           float* feat, int* tap_row, float* tap_w, float* lat, void* stream);
/* adjoint of the latent interpolation: d_latent_cl[tap_row][c] += tap_w * d_lat[col][c] (atomic; caller zero-fills) */
int diner_scatter_latent_grad_f32(const float* d_lat, const int* tap_row, const float* tap_w, long long cols,
                                  float* d_latent_cl, void* stream);
/* y (PC) = mean over nv slabs of x (nv, PC) (resnetfc.py:150-152); adjoint != 0: y (nv, PC) = x (PC) / nv */
int diner_view_mean_f32(const float* x, int nv, long long PC, float* y, int adjoint, void* stream);
/* db (N) += column sums of dY (M x N, row stride ld): bias gradients (caller zero-fills) */
int diner_colsum_f32(const float* dY, long long M, int N, int ld, float* db, void* stream);
/* dout == NULL: out (P,4) = [sigmoid(raw[:, :3]), relu(raw[:, 3])] (pixelnerf.py:139-143), raw has row stride ld;
 * dout (P,4) given: out (P, ld) = its adjoint with respect to raw (columns >= 4 zero) */
int diner_field_act_f32(const float* raw, const float* dout, long long P, int ld, float* out, void* stream);
/* adjoint of diner_composite_f32 with respect to the field values (nerf_renderer.py:299-301, :341-360):
 *   g_rgb (NR,3), g_depth (NR) or NULL -> d_field (NR,K,4).  z and rays carry no gradient (the sampler is no_grad).
 *   K <= 1024 (the range of diner_composite_long_f32; K <= 256 before the long entries). */
int diner_composite_bwd_f32(const float* field, const float* z, const float* rays, int NR, int K, int white_bkgd,
                            const float* g_rgb, const float* g_depth, float* d_field, void* stream);
/* adjoint of diner_composite_aux_f32: the same, plus g_alpha (NR) or NULL, the gradient of the ray's opacity alpha = sum_k w_k
 * (nerf_renderer.py:359), which adds g_alpha to every sample's G_k.  depth_var carries no gradient.  With g_alpha NULL the result is that
 * of diner_composite_bwd_f32 bit for bit.  New symbol, no ABI bump. */
int diner_composite_aux_bwd_f32(const float* field, const float* z, const float* rays, int NR, int K, int white_bkgd,
                                const float* g_rgb, const float* g_depth, const float* g_alpha, float* d_field, void* stream);

/* (n, HW, C) channels-last -> (n, C, HW): the latent gradient of diner_field_train_backward_f32 / diner_scatter_latent_grad_f32 in the
 * layout of the encoder's feature map (SpatialEncoder.latent, image_encoder.py:82-95), through LDS tiles. */
int diner_channels_last_to_nchw_f32(const float* src, int n, long long HW, int C, float* dst, void* stream);

/* The whole training forward / backward of the field for one object as one call each (the sequences of the building
 * blocks above that PixelNeRF.forward + ResnetFC.forward and their autograd adjoints amount to; pixelnerf.py:55-145,
 * resnetfc.py:129-159).  `params`: DEVICE parameter tensors in nn.Linear layout (d_in=55, d_latent=d_hidden=512, 5 blocks,
 * combine_layer=3); `workspace`: diner_field_train_workspace_bytes(P, nv) bytes, written by the forward (saved
 * pre-activations, taps, interpolated latent, the 13 weight matrices of the 512 x 512 layers packed in both orientations) and consumed
 * by the backward of the same call pair -- which therefore takes `params` with the VALUES the forward saw (an optimiser step belongs
 * after the backward); it also holds the backward's scratch (partial weight-gradient tiles: 13 x 33.6 MB).
 *   forward : xyz, viewdirs (P,3) -> out (P,4) = [sigmoid rgb, relu sigma]
 *   backward: d_out (P,4) -> `grads` (same structure as `params`, device buffers of the parameters' shapes, overwritten)
 *             and d_latent_cl (nv,Hf,Wf,512) or NULL (gradient of the channels-last feature map, overwritten). */
size_t diner_field_train_workspace_bytes(long long P, int nv);
int diner_field_train_forward_f32(const DinerScene* scene, const DinerMlpParams* params, const float* xyz,
                                  const float* viewdirs, long long P, float* out, void* workspace, void* stream);
int diner_field_train_backward_f32(const DinerScene* scene, const DinerMlpParams* params, const DinerMlpParams* grads,
                                   long long P, const float* d_out, void* workspace, float* d_latent_cl, void* stream);
/* Round 5: the workspace in two parts.  `saved_bytes`: what the forward leaves for the backward (per object: 10.8 GiB of the 15.4 at 4096
 * rays x 40 samples); `scratch_bytes`: the work buffers of either call (the backward's dx / dH / d_lat, partial weight-gradient tiles; the
 * forward's hand-over buffers) -- nothing in them lives from the forward to the backward, so the objects of a step, whose calls run one
 * after the other on a stream, can share ONE scratch buffer.  The _s entry points take the two parts separately (scratch NULL: the work
 * buffers follow the saved part in `workspace`, which then holds diner_field_train_workspace_bytes = saved + scratch bytes). */
int diner_field_train_workspace_split(long long P, int nv, size_t* saved_bytes, size_t* scratch_bytes);
int diner_field_train_forward_s_f32(const DinerScene* scene, const DinerMlpParams* params, const float* xyz, const float* viewdirs,
                                    long long P, float* out, void* workspace, void* scratch, void* stream);
int diner_field_train_backward_s_f32(const DinerScene* scene, const DinerMlpParams* params, const DinerMlpParams* grads, long long P,
                                     const float* d_out, void* workspace, void* scratch, float* d_latent_cl, void* stream);
/* Round 5 (the Python host uses it for objects with at least ~0.7 of a feature map of sample points; DINER_TRAIN_FUSED_FWD=1 / 0 forces it): the training forward on the INFERENCE kernels -- the f16x3
 * per-view and post kernels of diner_field_from_points_f32 in variants that store the pre-activations into the places of `workspace`
 * the layer-wise forward uses (diner_field_train_ws_layout), so that diner_field_train_backward_f32 follows unchanged.  `mlp`: the
 * packed-weights handle of THIS step's parameters.  latent_proj_out (diner_scene_proj_bytes; free again when the call's work is done):
 * the library projects scene->latent_cl through lin_z[0..2] into it on the training products' kernel (f16x3 with its bf16x6 repeat)
 * and gathers from it (round 6: only the texel rows the batch's taps name are projected -- a 64 x 64 ray patch touches 2-3 % of a 400 x 300 map;
 * the buffer must hold FINITE values before its first use (zero it once): a texel that another rounding of a tap's last bit would name is read
 * with a weight of ~1e-7; DINER_TRAIN_PROJ_TOUCHED=0: the whole map); NULL: `scene->latent_proj` prepared with `mlp` (diner_scene_prepare_f32) is used.  The exact repeat is the layer-wise
 * forward, enqueued by this call behind the fused kernels and gated on their range flag (no host synchronisation);
 * diner_field_train_fused_overflowed reads that flag back after a stream wait (a test aid).  DINER_E_UNSUPPORTED (weights outside the fp16
 * split, a projected map of 4 GiB or more): call diner_field_train_forward_f32 (pixelnerf.py:55-145, resnetfc.py:129-159). */
int diner_field_train_forward_fused_f32(const DinerScene* scene, const DinerMlp* mlp, const DinerMlpParams* p, const float* xyz,
                                        const float* viewdirs, long long P, float* out, void* workspace, void* scratch,
                                        float* latent_proj_out, void* stream);
int diner_field_train_fused_overflowed(const void* workspace, long long P, int nv, int* overflowed, void* stream);
/* ABI v6: the SB objects of a training step in ONE call pair (DINER.calc_losses renders SB = 4 objects x 4096 rays per step,
 * diner.py:217-290, configs/train_dtu.yaml:16,52-63; the reference's batched tensors (SB, B, ...) of pixelnerf.py:55-145 amount to this).
 * The ResnetFC layers are scene-independent: only the inputs / gather (forward) and the view-mean adjoint / latent-gradient scatter
 * (backward) are per object.  scenes: HOST array of n_obj scene pointers (same nv; same map sizes not required); xyz / viewdirs
 * (n_obj, P, 3), out / d_out (n_obj, P, 4), object-major.  `saved` / `scratch`: diner_field_train_batch_workspace_split bytes (the layout
 * of diner_field_train_workspace_split for n_obj * P points, rows object-major: diner_field_train_ws_layout(n_obj * P, nv) locates the saved
 * pre-activations).  forward: re-packs the PERSISTENT handle `mlp` from `p` (diner_mlp_update, training subset; no host synchronisation),
 * packs the step's 13 matrices once, then per object projects its latent map into latent_proj_scratch (the largest object's
 * diner_scene_proj_bytes; reused object after object) and runs the fused storing kernels with the gated layer-wise repeat behind them.
 * backward: the 13 x (data gradient, weight gradient) products ONCE over n_obj x P x nv rows -- n_obj times fewer launches, one partial-tile
 * sum, weight gradients of the step summed in-kernel -- then per object the scatter into d_latent_cl[o] (HOST array of n_obj device
 * pointers, entries or the array may be NULL).  map_scratch (or NULL): one map-shaped plane, diner_scene_proj_bytes / 3 bytes of the largest
 * object (the forward's latent_proj_scratch serves) -- with it the adjoint of the three lin_z terms runs in MAP space over the texel rows the
 * batch touches (dWz_b = D_b^T L, d latent = sum_b D_b Wz_b with D_b = the stream's gradient scattered through the bilinear taps) instead of
 * six products over the per-view sample rows; NULL: those products.  DINER_E_UNSUPPORTED as diner_field_train_forward_fused_f32 (before
 * anything is enqueued). */
int diner_field_train_batch_workspace_split(long long P, int nv, int n_obj, size_t* saved_bytes, size_t* scratch_bytes);
int diner_field_train_forward_batch_f32(const DinerScene* const* scenes, int n_obj, DinerMlp* mlp, const DinerMlpParams* p, const float* xyz,
                                        const float* viewdirs, long long P, float* out, void* saved, void* scratch,
                                        float* latent_proj_scratch, void* stream);
int diner_field_train_backward_batch_f32(const DinerScene* const* scenes, int n_obj, const DinerMlpParams* p, const DinerMlpParams* grads,
                                         long long P, const float* d_out, void* saved, void* scratch, float* const* d_latent_cl,
                                         float* map_scratch, void* stream);
/* Test aid: float offsets into the training workspace of the pre-activations the forward saved -- [0..4] X_b, the residual stream
 * entering block b (P*nv rows of 512 for b < 3, P rows behind the view mean), [5..9] H_b, the fc_0 outputs of block b, [10] the
 * stream entering lin_out (P x 512), [11] lin_out's raw outputs (P x 4).  The signs of these values are the relu decisions of the
 * forward (resnetfc.py:61-69): tests evaluate the reference's backward conditioned on them.  n >= 12. */
int diner_field_train_ws_layout(long long P, int nv, long long* float_offsets, int n);

/* ---- ABI v5: generic-shape slow path -------------------------------------------------------------------------------------------
 * ResnetFC.forward (resnetfc.py:129-159) for ANY configuration the reference's constructor accepts (resnetfc.py:72-127: d_hidden
 * default 128, any n_blocks / combine_layer / d_in / d_latent / d_out, Softplus for beta > 0; combine_type "average" is the only one
 * the reference implements, :9-14) and any number of views: the layers chained on the general exact-fp32 MFMA GEMM (diner_gemm_f32 with
 * its exact flag), one launch per layer, the mean over the views at block `combine_layer`.  The fused field kernels remain the path of
 * the shipped configuration; this one exists so that "same constructor kwargs" is "same behaviour" (training through it: the _train_
 * entry points below, ABI v6).  `p` holds DEVICE pointers to the parameters as nn.Linear stores them; no packing, no handle.
 *   zx   (nv, B, d_latent + d_in) row-major, the latent part first (resnetfc.py:140-142)
 *   out  (B, d_out) when 0 <= combine_layer < n_blocks (views averaged inside the network), else (nv, B, d_out)
 *   workspace: diner_mlp_generic_workspace_bytes(p, nv, B) bytes */
size_t diner_mlp_generic_workspace_bytes(const DinerMlpParams* p, int nv, long long B);
int diner_mlp_generic_forward_f32(const DinerMlpParams* p, float beta, const float* zx, int nv, long long B, float* out,
                                  void* workspace, void* stream);
/* ABI v6: training through the generic path (resnetfc.py:72-159 under torch autograd; e.g. ResnetFC's default d_hidden = 128).  The forward
 * keeps the pre-activations in `workspace` (diner_mlp_generic_train_workspace_bytes: (2 n_blocks + 1) saved tensors + three temporaries);
 * the backward chains data / weight / bias gradients, the adjoint of the view mean and -- when d_zx is not NULL -- the gradient with
 * respect to zx on the same exact-fp32 GEMM.  grads: device buffers of the parameters' shapes (overwritten).  n_blocks <= 64. */
size_t diner_mlp_generic_train_workspace_bytes(const DinerMlpParams* p, int nv, long long B);
int diner_mlp_generic_train_forward_f32(const DinerMlpParams* p, float beta, const float* zx, int nv, long long B, float* out,
                                        void* workspace, void* stream);
int diner_mlp_generic_backward_f32(const DinerMlpParams* p, const DinerMlpParams* grads, float beta, const float* zx, int nv, long long B,
                                   const float* d_out, void* workspace, float* d_zx, void* stream);
/* ... and the adjoint of the bilinear latent lookup of diner_field_inputs_generic_f32 (image_encoder.py:97-146 under autograd): d_latent_cl
 * (nv, Hf, Wf, C) channels-last, overwritten, from the first C columns of d_zx (nv, P, d_row); points given as xyz / viewdirs (P, 3). */
int diner_field_inputs_generic_bwd_f32(const DinerScene* scene, const float* xyz, const float* viewdirs, long long P, int d_row,
                                       const float* d_zx, float* d_latent_cl, void* stream);
/* The matrix PixelNeRF.forward hands to its MLP (pixelnerf.py:84-128) for any positional encoding / latent width / NV <= DINER_MAX_VIEWS:
 * zx (nv, P, C + d_in) with d_in = 4 (2 num_freqs + include_input) + 3, rows [latent (bilinear / border) ; poscode(x_c) ; R d ;
 * poscode(depth_nearest - z_c)].  Point source: (rays (NR,8), z (NR,K), K) with P = NR K, or (xyz, viewdirs) (P,3) with rays == NULL. */
int diner_field_inputs_generic_f32(const DinerScene* scene, const float* rays, const float* z, int K, const float* xyz,
                                   const float* viewdirs, long long P, int num_freqs, int include_input, float freq_factor,
                                   float* zx, void* stream);

/* ---- image-quality metrics (the reference's evaluate_folder, eval_suite.py:62-68) ----------------------------------------------
 * For N pairs of H x W images (H, W >= 7) writes out (N, 4) float64 = {l1, l2, psnr, ssim} per pair, in device memory:
 * a pixel value is the float32 fl32(k) / 255; l1 = mean |fl32(p - g)|, l2 = mean fl32(fl32(p - g)^2) (both summed in double),
 * psnr = 10 log10(1 / l2) (+inf when l2 == 0), ssim = skimage structural_similarity(channel_axis=-1, data_range=1) with its defaults
 * (7x7 uniform window, K1 0.01, K2 0.03, sample covariance, map cropped by 3 px, mean over the channels; moments and the map in double).
 * No floating-point atomics: the scores are bit-identical across runs, batch positions and the two routes.
 *   _u8:  pred (N,H,W,pred_c) with pred_c == 3, gt (N,H,W,gt_c) with gt_c 3 or 4 (alpha dropped), uint8;
 *   _f32: pred, gt (N,3,H,W) fp32, quantised in-kernel exactly as diner_quantize_rgb_u8 does (save_image).
 * workspace: diner_image_metrics_workspace_bytes(N, H, W) bytes of device memory (0 for arguments the entries refuse).
 * Bad arguments (null pointers, N < 1, H or W < 7, channel counts) return DINER_E_INVALID before any device work.
 * Added without an ABI bump: new symbols, no existing contract changed. */
size_t diner_image_metrics_workspace_bytes(int N, int H, int W);
int diner_image_metrics_u8(const unsigned char* pred, const unsigned char* gt, int N, int H, int W, int pred_c, int gt_c,
                           void* workspace, double* out, void* stream);
int diner_image_metrics_f32(const float* pred, const float* gt, int N, int H, int W, void* workspace, double* out, void* stream);

/* ---- the training objective (DINER.calc_losses around renderer.forward, reference src/models/diner.py:217-290) -------------------
 * New symbols without an ABI bump; enqueue-only on `stream`, no allocation, no host synchronisation, no floating-point atomics (the
 * outputs are bit-identical from run to run); bad arguments return DINER_E_INVALID before any device work.
 *
 * diner_sample_patch (diner.py:233-247): fg (SB,H,W) fp32 foreground weights (>= 0; a value that is not > 0 counts as 0), patch side s,
 *   u (SB) uniform numbers in [0, 1) or NULL -> Philox4x32-10 keyed by (seed, step, object).  With pad = (s + 1) / 2 the weights of the
 *   first and last pad rows and columns count as 0; the centre is the first pixel in row-major order whose inclusive prefix sum of
 *   weights (double; per-thread runs of consecutive pixels, then the threads in order) exceeds u * total.
 *   pix_idcs (SB, s*s) int32: the row-major block of pixels (cx - pad + j, cy - pad + i), i the slow index, as y * W + x;
 *   centres (SB,2) int32 (x, y); flags (SB) int32: 1 for an object whose padded mask is all zero (it gets the image centre
 *   (W / 2, H / 2)), else 0.  s + 1 > min(H, W) is refused.
 * diner_gen_rays_at_f32: diner_gen_rays_f32 at listed pixels: pix (B, n) int32 device (y * W + x) -> out (B, n, 8); a row is
 *   bit-identical to the row diner_gen_rays_f32 writes for that pixel.  Indices outside [0, W H) are clamped.  B <= 16 per call.
 * diner_objective_f32: losses (3) double = {rgb_fine, antibias, w_mse rgb_fine + w_antibias antibias} and d_pred (SB,B,3) fp32 = the
 *   gradient of losses[2] with respect to pred (SB,B,3).  Ground truth: gt (SB,B,3), or gt == NULL and images (SB,3,H,W) with
 *   pix (SB,B) int32 (gathered in the kernel, indices clamped; H, W unused with gt).
 *   rgb_fine = mean (p - g)^2 over SB B 3 values (MSELoss).  With a patch (s > 0, B == s*s, s a multiple of 2^n_downsampling, s <= 1024)
 *   D[o, ch, cell] = the mean of p - g over the 2^n x 2^n pixels of a cell of the patch viewed as (SB,3,s,s) (diner.py:281-282) and
 *   antibias = mean |D| (AntibiasLoss with L1Loss), gradient sign(D) / (4^n SB 3 (s / 2^n)^2) per pixel, sign(0) = 0.  s == 0 is the
 *   random-pixel mode (diner.py:229-230): antibias = 0 and w_antibias must be 0.  p - g rounds to fp32, every sum is double (partial
 *   sums per workgroup in `workspace`, diner_objective_workspace_bytes(SB, B, s, n_downsampling) bytes -- 0 for sizes the entry
 *   refuses -- added in a fixed order by a finalising launch).  w_mse = 1 is DINER's objective; w_mse = 0, w_antibias = 1 is
 *   AntibiasLoss alone. */
int diner_sample_patch(const float* fg, int SB, int H, int W, int s, const float* u, uint64_t seed, long long step, int* pix_idcs,
                       int* centres, int* flags, void* stream);
int diner_gen_rays_at_f32(const float* extrinsics, const float* intrinsics, const float* z_near, const float* z_far, int B,
                          int W, int H, const int* pix, long long n, float* out, void* stream);
size_t diner_objective_workspace_bytes(int SB, int B, int s, int n_downsampling);
int diner_objective_f32(const float* pred, const float* gt, const float* images, const int* pix, int SB, int B, int H, int W, int s,
                        int n_downsampling, double w_mse, double w_antibias, void* workspace, double* losses, float* d_pred,
                        void* stream);

/* ---- empty-ray culling: render only the rays the depth maps put a surface on ----------------------------------------------------
 * New symbols without an ABI bump; enqueue-only on `stream`, no allocation, no host synchronisation, no floating-point atomics, no
 * workgroup waiting on another (three launches, ordered by the stream); bad arguments return DINER_E_INVALID before any device work.
 *
 * diner_compact_live_f32: order-preserving stream compaction of one sampler batch, appended to a frame-level list.  stats (NR,4) as
 *   the info sampler entries write it ([1] = sum O, the reference's ray_mask of nerf_renderer.py:182 at threshold 0); ray i is LIVE iff
 *   !(stats[i][1] <= threshold), so a NaN is live.  With base = *n_live on entry (a device int32 the caller zeroes once per frame), the
 *   j-th live ray of the batch, in ray order, goes to row base + j: rays_out (capacity,8) and z_out (capacity,K) receive its rows of
 *   rays (NR,8) / z (NR,K), live_idx (capacity) int32 its frame index ray_index0 + i.  slot (NR) int32 receives the row of every ray of
 *   the batch, -1 for a dead ray and for a live one whose row is at or beyond `capacity` -- such rows are not written.  *n_live
 *   advances by the batch's true live count whatever the capacity: a counter above `capacity` tells the caller the list overflowed.
 *   The bytes written are a function of the inputs alone; a ray list split into consecutive calls gives those of the one call.
 *   1 <= K <= 1024; rows move as 16-byte vectors when K is a multiple of 4 and the bases are 16-byte aligned, as scalars otherwise.
 *   workspace: diner_compact_live_workspace_bytes(NR) bytes of device memory (0 for an NR the entry refuses).
 * diner_expand_live_f32: out (N,C) = slot[i] in [0, n_tiles) ? tiles[slot[i]] : bg, with tiles (n_tiles,C), slot (N) int32, bg (C)
 *   device; one coalesced pass, 1 <= C <= 8.  n_tiles == 0 (tiles may be NULL) fills the frame with bg. */
size_t diner_compact_live_workspace_bytes(long long NR);
int diner_compact_live_f32(const float* stats, float threshold, const float* rays, const float* z, int NR, int K, long long ray_index0,
                           long long capacity, float* rays_out, float* z_out, int* live_idx, int* slot, int* n_live, void* workspace,
                           void* stream);
int diner_expand_live_f32(const float* tiles, long long n_tiles, const int* slot, const float* bg, long long N, int C, float* out,
                          void* stream);

/* ---- geometry from a render: median / mean / z-depth, world points, cross-view depth consistency ----------------------------------
 * New symbols without an ABI bump (geometry.hip); enqueue-only on `stream`, one launch each, no allocation, no host synchronisation,
 * no atomics; bad arguments return DINER_E_INVALID with a message before any device work.
 *
 * diner_ray_geometry_f32: one reduction over weights (NR,K) as the compositor entries write them (nerf_renderer.py:351), the z (NR,K)
 *   and rays (NR,8) they were given; one wavefront per ray in the compositor's lane layout.  With w_k in sample order,
 *   c_k = sum_{j<=k} w_j (the lane's running sum + the wave scan of the lane totals before it) and A = c_{K-1}, the last element of that
 *   same sequence: a ray is VALID iff A > alpha_min (a NaN is invalid).  median_idx = min{k : c_k >= quantile * A} -- it exists because A
 *   is c_{K-1}, and "first k" keeps it defined where a weight is negative (a sample beyond `far`); depth_median = z[median_idx], on a
 *   surface where the mean of :356 lies between two; depth_mean = (sum_k w_k z_k) / A, the depth of :356 normalised by the opacity of
 *   :359; t = depth_median (point_mode 0) or depth_mean (point_mode 1); points (NR,3) = o + t d; zdepth = t (d . cam_fwd) with cam_fwd
 *   (host, 3 floats) row 2 of the target's world->camera rotation: the camera-z depth depth2normal.py:23-31 and the encoder take, where
 *   cam_geometry.py:33 normalises d and the depth of :356 is a distance along the ray.  An invalid ray writes 0 to every float output
 *   and -1 to median_idx (int32).  Any output pointer may be NULL; zdepth_out without cam_fwd is DINER_E_INVALID.
 *   NR >= 1, 1 <= K <= 1024, 0 < quantile <= 1, alpha_min >= 0.
 * diner_depth_consistency_f32: depth (N,H,W) device z-depth maps, 0 = no surface; intrinsics (N,3,3) and extrinsics (N,4,4)
 *   world->camera are HOST arrays (they travel as kernel arguments, 1 KiB); 2 <= N <= DINER_MAX_VIEWS.  Per reference view r and pixel
 *   (i, j) with D = depth[r][i][j] != 0, for every other view s: back-project ((j + 0.5 - cx) / fx D, (i + 0.5 - cy) / fy D, D), to
 *   world by R_r^T (X - t_r), into s; reject if z_s <= 0; project to (u, v), sample depth[s] bilinearly at (u - 0.5, v - 0.5) and reject
 *   unless all four taps are inside the image and non-zero; back-project (u, v) at the sampled depth from s and bring it into r: (u', v')
 *   and d'.  The pair is consistent iff hypot(u' - (j + 0.5), v' - (i + 0.5)) < px_thr and |d' - D| / D < rel_thr.  count (int32) = the
 *   consistent s, depth_avg = (D + sum of their d') / (count + 1); a pixel with D == 0 gets 0 and 0.  This is
 *   check_geometric_consistency / reproject_with_depth and the averaging of filter_depth (deps/TransMVSNet/dynamic_fusion.py) with one
 *   threshold pair, but with this project's pixel centres at +0.5 (depth2normal.py:23-31, cam_geometry.py:25-31) where that file uses
 *   integer pixels, and a tap rule stricter than its cv2.remap, which blends with zeros: the numbers are not its numbers bit for bit.
 *   Either output may be NULL. */
int diner_ray_geometry_f32(const float* weights, const float* z, const float* rays, int NR, int K, float quantile, float alpha_min,
                           const float* cam_fwd, int point_mode, float* depth_median_out, int* median_idx_out, float* depth_mean_out,
                           float* zdepth_out, float* points_out, void* stream);
int diner_depth_consistency_f32(const float* depth, const float* intrinsics, const float* extrinsics, int N, int H, int W, float px_thr,
                                float rel_thr, int* count_out, float* depth_avg_out, void* stream);

/* ---- surfaces: depth maps fused into a TSDF volume, and a triangle mesh out of it ---------------------------------------------------
 * New symbols without an ABI bump (surface.hip); no allocation, no atomics, no workgroup waiting on another (the stream is the only
 * ordering between launches); every output byte is a function of the inputs alone; bad arguments return DINER_E_INVALID with a
 * message before any device work.
 *
 * The volume is an axis-aligned box: sample (i, j, k) lies at origin + (i, j, k) voxel, origin (3 floats) on the HOST; each of Nx, Ny,
 * Nz is 2 .. 1024 and Nx Ny Nz < 2^31.  The device planes are (Nz, Ny, Nx) fp32, x fastest: tsdf (a fresh volume holds 1), wsum (0)
 * and optionally color4 (4, Nz, Ny, Nx) = sum w r, sum w g, sum w b, sum w (0).
 *
 * diner_tsdf_integrate_f32: one launch, enqueue-only, one thread per voxel; the voxel's values live in registers across a loop over the
 *   views IN VIEW ORDER, so the volume is read and written once per call whatever N, and one call with N views leaves the bits of N
 *   single-view calls in that order.  depth (N,H,W) device z-depth maps (camera z, the unit of predict_geometry's zdepth and of the
 *   source depth maps), weight (N,H,W) device or NULL (1 everywhere), color (N,3,H,W) device or NULL; intrinsics (N,3,3) and
 *   extrinsics (N,4,4) world->camera are HOST arrays (kernel arguments, 1 KiB); 1 <= N <= DINER_MAX_VIEWS.  Per view, with p the
 *   voxel's position: X = R p + t, skip unless X.z > 0; u = fx (X.x / X.z) + cx, v = fy (X.y / X.z) + cy, skip unless 0 <= u < W and
 *   0 <= v < H; the pixel is (floor v, floor u), the nearest with centres at +0.5; wp = weight there (or 1), skip unless wp > 0;
 *   D = depth there.  D > 0: sdf = D - X.z, skip if sdf < -trunc, d = min(1, sdf / trunc).  D == 0 with `carve`: d = 1 (the pixel is
 *   known to be empty: the whole ray is free space).  Anything else (D == 0 without carve, negative, NaN): skip.  Then
 *   tsdf = (tsdf wsum + d wp) / (wsum + wp) and wsum += wp, clamped to max_weight when max_weight > 0.  The colour sums take
 *   wp (r, g, b, 1) only where D > 0 and |sdf| <= trunc, and are never clamped.  color without color4, or the reverse, is refused.
 * diner_surface_workspace_bytes: device bytes diner_surface_count / _extract need for this volume (0 for dimensions they refuse).
 * diner_surface_count: two launches, enqueue-only: counts_out (device int32[2]) = the vertices and the quads of the naive surface
 *   nets mesh below; the workspace keeps the per-block offsets and the counts for diner_surface_extract_f32.
 * diner_surface_extract_f32: must follow diner_surface_count on the same stream with the same volume, min_weight and workspace, and
 *   be given the counts it wrote: it reads them back from the workspace (8 bytes, its one host synchronisation) and returns
 *   DINER_E_INVALID if they differ, before launching.  Two launches: vertices (+ the cell -> vertex map in the workspace), faces.
 *     A corner is NEGATIVE iff tsdf < 0 (an exact 0 and a NaN are positive) and OBSERVED iff wsum > min_weight.  Cell (i, j, k), i < Nx-1,
 *   j < Ny-1, k < Nz-1, is ACTIVE iff its 8 corners are observed and both signs occur.  One vertex per active cell, ids in linear cell
 *   order (x fastest): position = origin + voxel (cell + m), m = the mean over the sign-changing cell edges (a, b) of a + t (b - a),
 *   t = f_a / (f_a - f_b); normal = the normalised gradient of the trilinear interpolant of the 8 corner values at m -- towards
 *   increasing tsdf, free space -- or 0 where the gradient is 0; rgb (float) = trilinear(sum w c) / trilinear(sum w) at m, 0 where
 *   the denominator is not positive or color4 is NULL.  One quad per grid edge that starts at (i, j, k), runs to +x, +y or +z, changes
 *   sign and has its four neighbouring cells existing and active; quads in linear order of the start point, then x-, y-, z-edge; each
 *   starts at the neighbouring cell with the smallest indices and is wound so that its right-hand normal points from the negative to
 *   the positive end; triangles (0,1,2), (0,2,3).  An edge with a missing or inactive cell emits nothing: the mesh has a boundary there.
 *   vertices_out (nv,3), normals_out (nv,3) or NULL, rgb_out (nv,3) or NULL, faces_out (2 nq,3) int32. */
int diner_tsdf_integrate_f32(float* tsdf, float* wsum, float* color4, int Nx, int Ny, int Nz, const float* origin, float voxel,
                             float trunc, const float* depth, const float* weight, const float* color, const float* intrinsics,
                             const float* extrinsics, int N, int H, int W, int carve, float max_weight, void* stream);
size_t diner_surface_workspace_bytes(int Nx, int Ny, int Nz);
int diner_surface_count(const float* tsdf, const float* wsum, int Nx, int Ny, int Nz, float min_weight, void* workspace, int* counts_out,
                        void* stream);
int diner_surface_extract_f32(const float* tsdf, const float* wsum, const float* color4, int Nx, int Ny, int Nz, const float* origin,
                              float voxel, float min_weight, void* workspace, int n_vertices, int n_quads, float* vertices_out,
                              float* normals_out, float* rgb_out, int* faces_out, void* stream);

/* ---- ray-casting the TSDF volume: z-depth, normals, colour and confidence maps of any cameras ------------------------------------------
 * New symbols without an ABI bump (raycast.hip); no allocation, no LDS, no atomics, no barrier, one launch each, enqueue-only; every
 * output byte is a function of the inputs alone; bad arguments return DINER_E_INVALID with a message before any device work.
 *
 * The volume is the one above: sample (i, j, k) at origin + (i, j, k) voxel, origin (3 floats) on the HOST, planes (Nz, Ny, Nx) fp32;
 * a corner is OBSERVED iff wsum > min_weight and NEGATIVE iff tsdf < 0 (an exact 0 and a NaN are positive).
 *
 * diner_tsdf_raycast_f32: one thread per ray, a wavefront per 8 x 8 pixel tile.  intrinsics (V,3,3) and extrinsics (V,4,4) world->camera
 *   (R, t) are HOST arrays (kernel arguments), 1 <= V <= DINER_MAX_VIEWS.  Every fp32 operation below is rounded once, in this order.
 *     The ray of pixel (r, c): dcx = ((c + 0.5) - cx) / fx, dcy = ((r + 0.5) - cy) / fy, d_c = (dcx, dcy, 1);
 *   eye_a = -((R[0][a] t0 + R[1][a] t1) + R[2][a] t2); d_w,a = (R[0][a] dcx + R[1][a] dcy) + R[2][a]; the point at camera depth z is
 *   p_a(z) = eye_a + z d_w,a: the march is parametrised by camera z, the unit of the source depth maps.
 *     The samples sit on a lattice anchored at the camera: dz = step / sqrt((dcx dcx + dcy dcy) + 1), `step` a world length;
 *   z_n = (float)n dz for n = 1, 2, ... while z_n <= zfar -- a product, never a running sum.
 *     Sampling: g_a = (p_a(z_n) - origin_a) / voxel.  The sample is INSIDE iff 0 <= g_a <= N_a - 1 on every axis and z_n >= znear; its
 *   cell is min(floor g_a, N_a - 2) per axis and its fraction m_a = g_a - cell_a; it is OBSERVED iff it is inside and the 8 corners of
 *   the cell are observed; f_n = the trilinear interpolant of tsdf over the cell's corners at m, along x, then y, then z, each lerp as
 *   a + w (b - a).  (Sample 0, the eye, is never observed.)
 *     Termination: the first observed sample with f_n < 0 ends the march.  It is a HIT iff sample n - 1 was observed too (its f is then
 *   not negative); otherwise -- a solid met from behind, or out of unknown space -- and when the lattice runs out, the ray is a MISS.
 *     A hit's depth: z = z_(n-1) + dz (f_(n-1) / (f_(n-1) - f_n)).  Its attributes are taken at p(z), in the cell p(z) falls in
 *   (floor g clamped to 0 .. N - 2), with no observedness test there:
 *       normal = R n_w, n_w = grad / |grad| of the trilinear interpolant there (d/dx = the four x-differences of the corners, lerped along y
 *         then z; likewise y over (x, z) and z over (x, y); |grad| = sqrt((gx gx + gy gy) + gz gz); row a of R n_w =
 *         (R[a][0] n0 + R[a][1] n1) + R[a][2] n2): the camera frame, towards free space, hence facing the camera; 0 where |grad| is
 *         not positive;
 *       rgb = trilinear(sum w c) / trilinear(sum w), 0 where the denominator is not positive (diner_surface_extract_f32's rule);
 *       weight = trilinear(wsum).
 *   A miss writes 0 to every output.  zdepth_out (V,H,W); normal_out (V,3,H,W), rgb_out (V,3,H,W), weight_out (V,H,W) or NULL; rgb_out
 *   needs color4.  A NaN interpolant is not negative and does not end a march; as f_(n-1) it makes the hit's depth a NaN.
 *     Only the sample positions are fixed: a thread starts at the first lattice index that can be inside the box (a slab test widened
 *   by its own rounding), may stop past the exit, and -- given `bricks` -- jumps over lattice samples whose cell lies in a 0-brick,
 *   landing at or before the first sample outside it.  The terminating sample's predecessor is evaluated afresh, so the outputs with
 *   and without `bricks` are the same bits.  The loop is bounded by a trip count computed on the host: a call with more than 2^20
 *   lattice samples on any ray (zfar |d_c| / step at the steepest pixel) is refused, as are V outside 1 .. 16, a dimension outside
 *   2 .. 1024, voxel <= 0, step <= 0 or not finite, znear < 0, zfar not finite or <= znear, and a null required pointer.
 * diner_tsdf_bricks: bricks_out (device bytes, diner_tsdf_bricks_bytes of them) = one byte per brick of 8^3 cells, brick (bx, by, bz) at
 *   (bz nby + by) nbx + bx with nb_a = ceil((N_a - 1) / 8): 1 iff some cell of the brick has all 8 corners observed and at least one
 *   negative.  It must be built from the same planes and min_weight as the ray-cast that is given it.
 * diner_tsdf_bricks_bytes: the size of that buffer (0 for dimensions the entries refuse). */
size_t diner_tsdf_bricks_bytes(int Nx, int Ny, int Nz);
int diner_tsdf_bricks(const float* tsdf, const float* wsum, int Nx, int Ny, int Nz, float min_weight, unsigned char* bricks_out,
                      void* stream);
int diner_tsdf_raycast_f32(const float* tsdf, const float* wsum, const float* color4, int Nx, int Ny, int Nz, const float* origin,
                           float voxel, const unsigned char* bricks, const float* intrinsics, const float* extrinsics, int V, int H, int W,
                           float znear, float zfar, float step, float min_weight, float* zdepth_out, float* normal_out, float* rgb_out,
                           float* weight_out, void* stream);

/* ---- scoring clouds: nearest neighbour between two clouds through a uniform grid, and the sums the distance scores need ------------------
 * New symbols without an ABI bump (cloud.hip); no allocation, enqueue-only; no floating-point atomics: every output byte is a function of
 * the inputs alone (the order of the points inside a cell, which the integer atomics of the build decide, is never visible); bad
 * arguments return DINER_E_INVALID with a message naming the argument before any device work.
 *
 * The grid is built over a TARGET cloud xyz_b (NB,3) fp32 on the device, 1 <= NB < 2^31: a box at lo (3 floats on the HOST) of
 *   (Gx, Gy, Gz) cubic cells of side h, each side 1 .. DINER_CLOUD_MAX_DIM cells and at most DINER_CLOUD_MAX_CELLS in all.  The cell of a
 *   point is clamp(floor((p_a - lo_a) / h), 0, G_a - 1) per axis, each operation rounded in fp32; cell (i, j, k) is number
 *   (k Gy + j) Gx + i.  A target point with a non-finite coordinate goes into no cell and is never anybody's neighbour.
 * diner_cloud_grid_bytes: the size of the grid's workspace (0 for sizes the entries refuse).
 * diner_cloud_grid_build_f32: a counting sort of the target's indices by cell into `workspace` (16-byte aligned): count (32-bit integer
 *   atomics), exclusive scan, scatter through per-cell cursors.  The non-finite points are sorted behind the last cell, so the sorted
 *   indices -- NB int32 at byte diner_cloud_grid_order_offset of the workspace -- are a permutation of 0 .. NB - 1 in cell order.
 * diner_cloud_nearest_f32: one thread per query of xyz_a (NA,3), 1 <= NA < 2^31, against the grid built from the same xyz_b, lo, h and
 *   dims.  The squared distance to a target point is d2 = (dx dx + dy dy) + dz dz, every operation rounded in fp32.  A target point is a
 *   CANDIDATE iff d2 <= max_dist max_dist (the product rounded in fp32; max_dist > 0 or +inf).  Of two candidates the smaller d2 wins,
 *   equal d2 the smaller index.  d2_out (NA) is the winner's d2, idx_out (NA) its index in xyz_b; no candidate, or a query with a
 *   non-finite coordinate: idx -1, d2 +inf.  The search walks Chebyshev rings of cells around the query's (unclamped) cell and stops
 *   once no unvisited cell can hold a candidate that beats the best found -- a bound evaluated in double and shrunk by more than the
 *   binning's rounding -- so the outputs equal exhaustive search bit for bit whatever the box and the cell size.  `order` (NA int32 on
 *   the device, or NULL) is the order in which the threads take the queries: thread t answers query order[t] (entries outside
 *   0 .. NA - 1 are skipped); it must be a permutation and changes no output.
 * diner_cloud_reduce_f32: over the n entries of (d2, idx) that are MATCHED -- idx >= 0 and d2 <= max_dist max_dist -- out (device,
 *   DINER_CLOUD_REDUCE_OUT doubles) = { the number matched, the sum of sqrt((double)d2), the sum of |n_a[i] . n_b[idx[i]]| (the dot
 *   product in double, (x + y) + z; 0 unless both normal arrays, (n,3) and (nb_rows,3), are given; an index >= nb_rows adds 0), then per threshold
 *   t < T <= 8 the number matched with d2 <= tau_t tau_t (fp32 product; thresholds: T floats on the HOST) }.  Sums run per thread in index
 *   order, then over the workgroup, then over the workgroups in a fixed order: two runs give the same bits.  workspace:
 *   diner_cloud_reduce_workspace_bytes(n) bytes (0 for n < 1). */
#define DINER_CLOUD_MAX_DIM 1024
#define DINER_CLOUD_MAX_CELLS (1 << 26)
#define DINER_CLOUD_MAX_THRESHOLDS 8
#define DINER_CLOUD_REDUCE_OUT (3 + DINER_CLOUD_MAX_THRESHOLDS)
size_t diner_cloud_grid_bytes(long long NB, int Gx, int Gy, int Gz);
size_t diner_cloud_grid_order_offset(long long NB, int Gx, int Gy, int Gz);
int diner_cloud_grid_build_f32(const float* xyz_b, long long NB, const float* lo, float h, int Gx, int Gy, int Gz, void* workspace,
                               void* stream);
int diner_cloud_nearest_f32(const float* xyz_b, long long NB, const float* lo, float h, int Gx, int Gy, int Gz, const void* workspace,
                            const float* xyz_a, long long NA, const int* order, float max_dist, float* d2_out, int* idx_out, void* stream);
size_t diner_cloud_reduce_workspace_bytes(long long n);
int diner_cloud_reduce_f32(const float* d2, const int* idx, long long n, float max_dist, const float* thresholds, int T,
                           const float* normals_a, const float* normals_b, long long nb_rows, void* workspace, double* out,
                           void* stream);

/* ---- the perceptual network: the VGG convolution stack behind LPIPS and the VGG loss ----------------------------------------------------
 * New symbols without an ABI bump (perceptual.hip); no allocation, enqueue-only, everything fp32; activations are channels-last
 * (N,H,W,C) on the device; no floating-point atomics: every sum runs in an order the sizes alone fix, so two runs give the same bits
 * and an image's values do not depend on its place in the batch.  Bad arguments return DINER_E_INVALID before any device work.
 * Non-finite inputs are the caller's error: the result is unspecified, nothing faults.
 *
 * diner_conv3x3_f32: y = conv(x, w) + bias, 3 x 3, stride 1, zero padding 1, any Cin, Cout >= 1, N <= 65535; then, in this order,
 *   + addend (N,H,W,Cout) if given, ReLU if relu != 0, zero where !(mask > 0) if mask (N,H,W,Cout) is given.  An implicit GEMM on
 *   v_mfma_f32_16x16x4_f32: every output is one fp32 fmaf chain that starts at the bias and runs over the input channels in chunks of
 *   DINER_CONV3X3_CIN_CHUNK, inside a chunk over the nine taps row-major, inside a tap over the chunk's channels.
 *   wpack: diner_conv3x3_pack_floats(Cin, Cout) floats, 16-byte aligned, [ceil(Cin / 8)][tap ky 3 + kx][8][CoutPad] with CoutPad = Cout
 *   rounded up to DINER_CONV3X3_COUT_TILE and element = w[cout][cin][ky][kx] of a torch Conv2d weight, zeros beyond Cin and Cout; bias:
 *   CoutPad floats or NULL.  The data gradient of that convolution is the same call on the gradient with the weight set packed from
 *   w'[cin][cout][ky][kx] = w[cout][cin][2 - ky][2 - kx]; addend and mask are its epilogue: the loss gradient that enters at the
 *   activation below, and that activation's ReLU mask.  A call with Cin = 4 on a weight packed for Cin = 3 is valid (same layout).
 * diner_maxpool2_f32: torch's MaxPool2d(2, 2): y (N, H / 2, W / 2, C), odd sizes floored; H, W >= 2.
 * diner_maxpool2_bwd_f32: gx (N,H,W,C) from gy (N, H / 2, W / 2, C) and the saved input x: the gradient goes to the first maximum of
 *   each window in row-major order (a later value wins only if greater, or a NaN), everything else gets 0; then + addend (N,H,W,C) if
 *   given, then zero where !(x > 0) if relu_mask != 0.
 * diner_image_in_f32: x (N,3,H,W) -> y (N,H,W,Cs), y = (x - shift[c]) / scale[c], each operation rounded in fp32; Cs is 3, or 4 with
 *   a zero fourth channel; shift and scale are three floats on the HOST.  diner_image_in_bwd_f32: its adjoint, gx (N,3,H,W) =
 *   g (N,H,W,Cs)[..., c] / scale[c].
 * diner_feature_l1_f32: out[0] (device double) = mean |fx - fy| over n elements, the differences (exact) and their sum in double: per
 *   thread in index order, then over the workgroup, then over the workgroups in order.  grad (n floats, or NULL) = g sign(fx - fy) with
 *   g = (float)(weight / n), and 0 where !(fx > 0) if mask_by_fx != 0.  workspace: diner_feature_l1_workspace_bytes(n) bytes.
 * diner_lpips_layer_f32: per image i < N, out[i] (device doubles) = [out[i] +, if accumulate != 0] the mean over the HW pixels of
 *   sum_c lin[c] (fx_c / (sqrt(sum fx^2) + 1e-10) - fy_c / (sqrt(sum fy^2) + 1e-10))^2, fx, fy (N,HW,C), all arithmetic in double, the
 *   sums in a fixed order per image.  workspace: diner_lpips_layer_workspace_bytes(N, HW) bytes. */
#define DINER_CONV3X3_CIN_CHUNK 8
#define DINER_CONV3X3_COUT_TILE 64
size_t diner_conv3x3_pack_floats(int Cin, int Cout);
int diner_conv3x3_f32(const float* x, const float* wpack, const float* bias, const float* addend, const float* mask, float* y, int N, int H,
                      int W, int Cin, int Cout, int relu, void* stream);
int diner_maxpool2_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
int diner_maxpool2_bwd_f32(const float* x, const float* gy, const float* addend, int relu_mask, float* gx, int N, int H, int W, int C,
                           void* stream);
int diner_image_in_f32(const float* x, const float* shift, const float* scale, float* y, int N, int H, int W, int Cs, void* stream);
int diner_image_in_bwd_f32(const float* g, const float* scale, float* gx, int N, int H, int W, int Cs, void* stream);
size_t diner_feature_l1_workspace_bytes(long long n);
int diner_feature_l1_f32(const float* fx, const float* fy, long long n, double weight, int mask_by_fx, float* grad, void* workspace,
                         double* out, void* stream);
size_t diner_lpips_layer_workspace_bytes(int N, long long HW);
int diner_lpips_layer_f32(const float* fx, const float* fy, const float* lin, int N, long long HW, int C, int accumulate, void* workspace,
                          double* out, void* stream);

/* ---- the optimiser step: Adam / AdamW over all parameter tensors in one launch -----------------------------------------------------------
 * New symbols without an ABI bump (optim.hip); no allocation, everything fp32; the two device entries are enqueue-only, the two table
 * entries are host-only arithmetic.  Bad arguments return DINER_E_INVALID (the byte count: 0) with a message before any device work.
 *
 * The chunk table.  n records DinerOptimTensor {param, grad, exp_avg, exp_avg_sq, numel} (device addresses; never dereferenced on the
 *   host) become n_chunks records DinerOptimChunk: each covers at most DINER_OPTIM_CHUNK elements of ONE tensor, the chunks of a tensor
 *   tile it once, in order, in record order, and every chunk but a tensor's last holds exactly DINER_OPTIM_CHUNK elements -- a multiple of
 *   4, so a chunk's pointers are 16-byte aligned exactly where the tensor's base pointers are.  A record with numel == 0 contributes no
 *   chunk; n <= 0, numel < 0 or a null pointer in a record with numel > 0 is refused.  The table buffer is the n_chunks chunk records
 *   followed by n_chunks 16-byte slots {double sum of squares, int64 non-finite count} that the statistics pass writes (zeroed by the
 *   build); the table-bytes entry gives the size of both together.  The build fills a caller-provided HOST buffer of that size, which
 *   the caller uploads (a stream-ordered copy from pinned memory) to a device buffer of the same size.
 * The state block.  DinerOptimState, 64 bytes on the device, zero before the first step.  step and skipped have two slots: a step launched
 *   with DinerAdamHyper.slot = s reads slot s and writes slot s ^ 1 (no workgroup reads what the launch writes), so the caller passes
 *   slot = (number of step launches so far) & 1 and reads the result from the other slot.  The step count lives here, not on the host,
 *   because a skipped step does not advance it.
 * diner_optim_grad_stats: grad_norm_sq = the sum of (double)g^2 over all gradients of the table, nonfinite = the number of gradient elements
 *   that are inf or NaN (they enter the sum: the norm is then non-finite, as torch's).  Two launches: per-chunk partials (per thread in index
 *   order, the lanes' xor tree, the waves in order), then one workgroup adds the partials in table order.  No atomics, no waiting between
 *   workgroups: the bits are a function of the table and the values only.  Needed before a step with CLIP or SKIP_NONFINITE.
 * diner_adam_step_f32: torch.optim.Adam's single-tensor update per element, each operation rounded in fp32 as torch's kernels round it,
 *     g *= clip;  g += wd p  (or p *= 1 - lr wd with DINER_ADAM_DECOUPLED_WD: AdamW);  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
 *     p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps),      t = step[slot] + 1, the corrections in double on the device.
 *   DINER_ADAM_CLIP: clip = min(1, max_norm / (sqrt(grad_norm_sq) + 1e-6)), torch's clip_grad_norm_; otherwise 1.
 *   DINER_ADAM_SKIP_NONFINITE: with nonfinite != 0 nothing is written but skipped[slot ^ 1] = skipped[slot] + 1, step[slot ^ 1] = step[slot],
 *     clip = 0 and, with DINER_ADAM_ZERO_GRADS, the zeroed gradients; p, m and v keep their bits.
 *   DINER_ADAM_ZERO_GRADS: every gradient element is overwritten with 0 after it has been read.
 *   Chunks whose four pointers are 16-byte aligned move 16 bytes per lane and access, with numel % 4 scalar elements at a tensor's end; a
 *   chunk with a pointer off that boundary is processed element by element. */
#define DINER_OPTIM_CHUNK 4096
typedef struct DinerOptimTensor {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long numel;
} DinerOptimTensor;
typedef struct DinerOptimChunk { /* 48 bytes */
  float* param;                  /* the chunk's first element of each of the four arrays */
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int32_t numel;                 /* 1 .. DINER_OPTIM_CHUNK */
  int32_t tensor;                /* index of the record the chunk belongs to */
  long long offset;              /* of the chunk's first element in its tensor */
} DinerOptimChunk;
typedef struct DinerOptimState { /* 64 bytes, device */
  long long step[2];             /* completed (not skipped) steps */
  long long skipped[2];          /* steps skipped for a non-finite gradient */
  double grad_norm_sq;           /* of the last statistics pass */
  long long nonfinite;           /* of the last statistics pass */
  double clip;                   /* factor the last step applied to the gradients (0: skipped) */
  long long reserved;
} DinerOptimState;
#define DINER_ADAM_DECOUPLED_WD   1u
#define DINER_ADAM_CLIP           2u
#define DINER_ADAM_SKIP_NONFINITE 4u
#define DINER_ADAM_ZERO_GRADS     8u
#define DINER_ADAM_ALL_FLAGS      15u
typedef struct DinerAdamHyper {  /* host */
  double lr, beta1, beta2, eps, weight_decay, max_norm;
  uint32_t flags;
  int32_t slot;
} DinerAdamHyper;
size_t diner_optim_table_bytes(const DinerOptimTensor* t, int n);
int diner_optim_table_build(const DinerOptimTensor* t, int n, void* host_out, size_t bytes, int* n_chunks);
int diner_optim_grad_stats(void* table, int n_chunks, DinerOptimState* state, void* stream);
int diner_adam_step_f32(const void* table, int n_chunks, DinerOptimState* state, const DinerAdamHyper* hyper, void* stream);

/* ---- the image encoder's trunk: the ResNet feature pyramid behind DinerScene.latent_cl ---------------------------------------------------
 * New symbols without an ABI bump (encoder.hip); no allocation, enqueue-only, everything fp32; activations are channels-last (N,H,W,C) on
 * the device.  Every output is computed in an order the shape alone fixes and no tile crosses images, so an image's values are the same
 * bits at any place in the batch.  Bad arguments return DINER_E_INVALID (a kernel size that is not built: DINER_E_UNSUPPORTED) with a
 * message before any device work.  Together with diner_conv3x3_f32 (addend = the block's identity) these are SpatialEncoder.forward in
 * eval mode, BatchNorm folded into the convolutions: w' = w s, b' = beta - mean s, s = gamma / sqrt(var + eps).
 *
 * diner_conv2d_s2_f32: y[..., coff + o] = conv(x, w)[o] + bias[o], R x R with R in {1, 3, 7}, stride 2, zero padding R / 2, any Cin,
 *   Cout >= 1, N <= 65535; then ReLU if relu != 0.  x (N,H,W,Cin); y (N,Ho,Wo,ldy) with Ho = (H + 2 (R / 2) - R) / 2 + 1 (Wo likewise), of
 *   which only channels coff .. coff + Cout - 1 are written (ldy = Cout, coff = 0: a dense output).  An implicit GEMM on
 *   v_mfma_f32_16x16x4_f32: every output is one fp32 fmaf chain that starts at the bias and runs over the input channels in chunks of
 *   DINER_CONV3X3_CIN_CHUNK, inside a chunk over the kernel rows, inside a row over the kernel columns, inside a tap over the chunk's
 *   channels.  wpack: diner_conv2d_s2_pack_floats(Cin, Cout, R) floats (0 for arguments the convolution refuses), 16-byte aligned,
 *   [ceil(Cin / 8)][tap ky R + kx][8][CoutPad], CoutPad = Cout rounded up to DINER_CONV3X3_COUT_TILE, element = w[cout][cin][ky][kx] of a
 *   torch Conv2d weight, zeros beyond Cin and Cout -- for R = 3 the layout of diner_conv3x3_pack_floats.  bias: Cout floats or NULL.
 *   With Cin a multiple of 4 and x 16-byte aligned the input is read 16 bytes at a time, else element by element: a caller with 21 (or 3)
 *   input channels does better to let diner_encoder_input_f32 write 24 (4) and to pack the weights for that Cin -- the zero channels add
 *   exact zeros, the result is the same bits.
 * diner_maxpool3s2_f32: torch's MaxPool2d(3, 2, 1): y (N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C) dense, from x (N,H,W,ldx) of which channels
 *   0 .. C - 1 are read (ldx >= C; ldx = C: a dense input).  The padding is -inf, not 0; a NaN in a window is its result.
 * diner_encoder_input_f32: x (N,3,H,W) -> y (N, H + 2 pad, W + 2 pad, C): channels 0 .. 2 the image, replication-padded by pad;
 *   channels 3 .. 3 + Cring - 1 a copy of ring (H + 2 pad, W + 2 pad, Cring), the positional encoding of the padding ring (zero inside
 *   the image), the same for every image; channels beyond that zero.  C >= 3 + Cring; pad = 0, Cring = 0, C = 3 is a plain relayout.
 * diner_pyramid_level_f32: bilinear resampling with align_corners = True (torch's F.interpolate; evaluated in double, rounded once) of x (N,h,w,c) to
 *   Hf x Wf, written to channels c0 .. c0 + c - 1 of y (N,Hf,Wf,Ctot); no other channel is touched.  Source coordinate
 *   dst (h - 1) / (Hf - 1), scale 0 when Hf = 1.  h = Hf and w = Wf is a copy, bit for bit.  N, Hf <= 65535.  With c, Ctot and c0 multiples
 *   of 4 and both pointers 16-byte aligned it moves 16 bytes per access, else 4.
 *
 * A torch-free caller's sequence from four normalised images to DinerScene.latent_cl is in INTEGRATION.md ("Encoding source views"). */
size_t diner_conv2d_s2_pack_floats(int Cin, int Cout, int R);
int diner_conv2d_s2_f32(const float* x, const float* wpack, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int R, int relu,
                        int ldy, int coff, void* stream);
int diner_maxpool3s2_f32(const float* x, float* y, int N, int H, int W, int C, int ldx, void* stream);
int diner_encoder_input_f32(const float* x, const float* ring, float* y, int N, int H, int W, int pad, int Cring, int C, void* stream);
int diner_pyramid_level_f32(const float* x, float* y, int N, int h, int w, int c, int Hf, int Wf, int Ctot, int c0, void* stream);

/* ---- the depth estimator's matching stage: cost volume, depth read-out, next-stage hypotheses ------------------------------------------
 * New symbols without an ABI bump (mvs.hip); inference only, no allocation, enqueue-only, no host read-back, everything fp32.  They are
 * what TransMVSNet's DepthNet.forward and the stage loop of TransMVSNet.forward do between the learned networks (FeatureNet / FMT before,
 * CostRegNet in the middle, which stay with the caller).  No atomics; the order of every sum is fixed by the shape alone and no workgroup
 * crosses samples, so a sample's values are the same bits at any place in the batch.  Bad arguments and sizes beyond the limits return
 * DINER_E_INVALID with a message before any device work; nothing is truncated.
 *
 * diner_mvs_cost_volume_f32: the view-weighted feature similarity of a reference view against NS source views over D per-pixel depth
 *   hypotheses, without the warped (B,C,D,H,W) volume or a sampling grid.
 *     ref_cl (B,H,W,C), src_cl (NS,B,H,W,C): channels-last feature maps, 16-byte aligned.  proj (B,NS+1,2,4,4): per view the pair
 *     (extrinsics 4x4, intrinsics in the top-left 3x3 of the second 4x4), view 0 the reference.  depth (B,D,H,W).  Exactly one of
 *     pixelwise (DINER_MVS_PIXELWISE_FLOATS floats, below) and view_weights_in (B,NS,H,W) is non-NULL.  similarity (B,D,H,W) out [the
 *     reference's (B,1,D,H,W)]; view_weights_out (B,NS,H,W) out, required with pixelwise, else unused.  homography: B NS 12 floats of
 *     workspace.
 *   Per (b, source view v) a prep kernel computes proj = (K_s E_s[:3,:4] ; 0 0 0 1) inverse(K_r E_r[:3,:4] ; 0 0 0 1) in double (3x3
 *   adjugate) and rounds rot = proj[:3,:3] | trans = proj[:3,3] once to 12 floats.  Per (pixel x,y; depth d):
 *   p = (rot (x, y, 1)) depth[b,d,y,x] + trans; p.z < 1e-6: the sample is a zero feature; else the source map is sampled at
 *   (p.x / p.z, p.y / p.z) in pixel units, bilinear, zero padding (a tap outside the map adds 0, the others keep their weights; NaN
 *   coordinates sample 0).  similarity_v[d] = (sum_c warped[c] ref[c]) / C, each tap's dot product an fmaf chain over c in order, the
 *   taps combined in the order (x0,y0), (x1,y0), (x0,y1), (x1,y1).  View weight: w_v = max_d sigmoid(net(similarity_v[d])) with net the
 *   1 -> 16 -> 8 -> 1 pointwise net, BatchNorm folded: pixelwise = w0[16] b0[16] w1[8][16] b1[8] w2[8] b2, h0 = relu(w0 s + b0),
 *   h1 = relu(w1 h0 + b1), y = w2 h1 + b2, sigmoid = 1 / (1 + exp(-y)) -- a view whose samples all fall outside gets
 *   max_d sigmoid(net(0)) -- or w_v = view_weights_in[b,v,y,x].  similarity[d] = (sum_v similarity_v[d] w_v) / (1e-5 + sum_v w_v), views
 *   in order.
 *   Limits: 1 <= NS <= DINER_MAX_VIEWS - 1, C a multiple of 4 in [4, DINER_MVS_MAX_CHANNELS], 1 <= D <= DINER_MVS_MAX_DEPTHS, any
 *   B, H, W >= 1 with B D H W < 2^31.
 * diner_mvs_select_depth_f32: cost (B,D,H,W) [+ prob_init (B,D,H,W) or NULL, added first]; per pixel prob = exp(log_softmax(cost)) along D
 *   (maximum subtracted, the sum in d order), arg = the first index of the maximum of prob, depth (B,H,W) = hypotheses[b,arg,y,x],
 *   confidence (B,H,W) = prob[arg]; prob_volume (B,D,H,W) is written when non-NULL.  D >= 1, B D H W < 2^31.
 * diner_mvs_hypotheses_f32: the next stage's hypotheses (B, D, H / scale, W / scale) from the previous stage's depth cur_depth (B,h,w), equal
 *   to torch's chain F.interpolate(cur, (H,W), bilinear, align_corners=False) -> lo = up - half_range, hi = up + half_range,
 *   step = (hi - lo) / (D - 1), sample_d = lo + d step -> F.interpolate(., (D, H / scale, W / scale), trilinear, align_corners=False),
 *   which is the identity along d and two taps per axis in the plane (the 2 x 2 mean at scale 2; at scale 4 the mean of the window's
 *   CENTRE 2 x 2, not of all 16 -- torch does not low-pass), in one pass.  half_range = ndepth / 2 * interval.  scale in {1, 2, 4},
 *   2 <= D <= DINER_MVS_MAX_DEPTHS, integer division of H and W as the reference does. */
#define DINER_MVS_PIXELWISE_FLOATS 177
#define DINER_MVS_MAX_DEPTHS 256
#define DINER_MVS_MAX_CHANNELS 64
int diner_mvs_cost_volume_f32(const float* ref_cl, const float* src_cl, const float* proj, const float* depth, const float* pixelwise,
                              const float* view_weights_in, float* similarity, float* view_weights_out, float* homography, int B, int NS, int C,
                              int D, int H, int W, void* stream);
int diner_mvs_select_depth_f32(const float* cost, const float* prob_init, const float* hypotheses, float* depth, float* confidence,
                               float* prob_volume, int B, int D, int H, int W, void* stream);
int diner_mvs_hypotheses_f32(const float* cur_depth, float* hypotheses, int B, int h, int w, int H, int W, int scale, int D, float half_range,
                             void* stream);

/* ---- the matching stage in training: the per-view similarity and its backward pass ---------------------------------------------------
 * New symbols without an ABI bump (mvs.hip); layouts, limits, checks and the tap geometry are diner_mvs_cost_volume_f32's (the geometry
 * is one function, csrc/mvs_geom.hpp, that restates that kernel's operations in its order).  No gradient goes to depth, proj or the view
 * weights: the reference computes the sampling positions under no_grad.
 *
 * diner_mvs_similarity_f32: similarity (B,NS,D,H,W) out, similarity[b,v,d] = similarity_v[d] above -- the bits diner_mvs_cost_volume_f32
 *   aggregates.  homography (B NS 12 floats) out: hand it to the backward pass.
 * diner_mvs_similarity_grad_f32: the gradients of sum_{b,v,d,pixel} G similarity at the feature maps.  The upstream gradient is either
 *   grad_views (B,NS,D,H,W) = G, or grad_aggregated (B,D,H,W) = g with view_weights (B,NS,H,W) = w, from which the kernel forms
 *   G_v = g w_v / (1e-5 + sum_v w_v) (the sum in view order) without an NS-fold volume; the other form's pointers are NULL.
 *   homography: what the forward entry (either of the two) wrote.
 *   d_ref (B,H,W,C) = (1/C) sum_v sum_d G_vd sum_tap bw_tap src[v,tap,:]: no atomics, a pixel's partial sums are added in an order the
 *   shape alone fixes, every element is written; the same bits on every run and at any place in the batch.
 *   d_src (NS,B,H,W,C) += (1/C) G_vd bw_tap ref[pixel,:] at each tap: zeroed by one hipMemsetAsync here, then float atomic adds, whose
 *   order is not fixed (the last bits may differ between runs).  A tap whose G bw is exactly 0 adds nothing to either. */
int diner_mvs_similarity_f32(const float* ref_cl, const float* src_cl, const float* proj, const float* depth, float* similarity,
                             float* homography, int B, int NS, int C, int D, int H, int W, void* stream);
int diner_mvs_similarity_grad_f32(const float* ref_cl, const float* src_cl, const float* homography, const float* depth,
                                  const float* grad_views, const float* grad_aggregated, const float* view_weights, float* d_ref,
                                  float* d_src, int B, int NS, int C, int D, int H, int W, void* stream);

/* ---- the depth estimator's cost regulariser: the layers of CostRegNet, a 3-D U-Net of 3 x 3 x 3 convolutions ---------------------------
 * New symbols without an ABI bump (costreg.hip); inference only, no allocation, enqueue-only, one launch each, everything fp32;
 * activations are channels-last (N,D,H,W,C) on the device -- a one-channel volume (N,1,D,H,W) is that layout already.  No atomics; every
 * output is a sum of fp32 fmaf chains (v_mfma_f32_16x16x4_f32; plain fmaf in the same order where a stride-1 layer has Cin 1 and Cout <= 16,
 * or Cout 1 and Cin 4 or 8) whose order the shape alone fixes, and no workgroup crosses samples, so two runs give the same bits and a
 * sample's values do not depend on its place in the batch.  Bad arguments return DINER_E_INVALID with a message
 * before any device work.  Non-finite inputs are the caller's error: the result is unspecified, nothing faults.
 *
 * diner_conv3d_f32: y = conv(x, w) + bias, 3 x 3 x 3, stride 1 or 2, zero padding 1, any Cin, Cout >= 1, N <= 65535; the output has
 *   (n - 1) / stride + 1 voxels per axis (odd sizes are legal at stride 2).  Then, IN THIS ORDER, ReLU if relu != 0, then + addend
 *   (N,Do,Ho,Wo,Cout) if given: the U-Net adds its skip tensors after the activation.  This is NOT diner_conv3x3_f32's order (addend, then
 *   ReLU).  y may be the addend; it must not overlap x.
 *   An output is bias + s_0 + s_1 + ..., added in that order, with s_c the sum over chunk c of DINER_CONV3D_CIN_CHUNK input channels: one
 *   fmaf chain from zero over the 27 taps in (kd, kh, kw) row-major order, inside a tap over the chunk's channels (zeros beyond Cin and
 *   outside the volume take part: they add +0).  One chain per chunk, not one per output, keeps the rounding error of Cin 64 (1728
 *   products) near that of Cin 8.
 *   wpack: diner_conv3d_pack_floats(Cin, Cout) floats, 16-byte aligned, [ceil(Cin / 8)][tap (kd 3 + kh) 3 + kw][8][CoutPad], element =
 *   w[cout][cin][kd][kh][kw] of a torch Conv3d weight, zeros beyond Cin and Cout; CoutPad = 16 for Cout <= 16, 32 for Cout <= 32, else
 *   Cout rounded up to 64 (the kernels run one, two or four DINER_CONV3D_COUT_TILE-wide column tiles a workgroup).  bias: Cout floats
 *   (not padded) or NULL.  diner_conv3d_pack_floats returns 0 for Cin < 1 or Cout < 1.
 * diner_deconv3d_s2_f32: torch's ConvTranspose3d(3, stride 2, padding 1, output_padding 1): y (N, 2 D, 2 H, 2 W, Cout) from
 *   x (N,D,H,W,Cin), computed as a gather: per axis output index o receives input i through tap k = o + 1 - 2 i -- an even o from
 *   (k 1, i o / 2), an odd o from (k 0, i (o + 1) / 2) and (k 2, i (o - 1) / 2), an i beyond the input adding zero.  Same epilogue, same
 *   sums (per chunk a chain over the taps the output's parity class has in (kd, kh, kw) order, then channel) and the same pack layout, with
 *   element = w[cin][cout][kd][kh][kw] of the torch ConvTranspose3d weight (no flip). */
#define DINER_CONV3D_CIN_CHUNK 8
#define DINER_CONV3D_COUT_TILE 16
size_t diner_conv3d_pack_floats(int Cin, int Cout);
int diner_conv3d_f32(const float* x, const float* wpack, const float* bias, const float* addend, float* y, int N, int D, int H, int W, int Cin,
                     int Cout, int stride, int relu, void* stream);
int diner_deconv3d_s2_f32(const float* x, const float* wpack, const float* bias, const float* addend, float* y, int N, int D, int H, int W,
                          int Cin, int Cout, int relu, void* stream);

/* ---- the depth estimator's feature transformer: TransMVSNet's FMT and its FPN pathway --------------------------------------------------
 * New symbols without an ABI bump (fmt.hip); inference only, no allocation, enqueue-only, everything fp32 (the partial sums of the
 * attention state are doubles); activations are channels-last tokens (N, L = H W, 32).  Built for d_model DINER_FMT_D_MODEL, DINER_FMT_NHEAD
 * heads, d_ff DINER_FMT_D_FF and maps of at most DINER_FMT_MAX_HW a side.  No atomics; every sum has an order the shape alone fixes and no
 * workgroup crosses images, so two runs give the same bits and an image's values depend neither on its place in the batch nor on how
 * many images share the call.  Bad arguments return DINER_E_INVALID with a message before any device work.
 *
 * The layer pack, diner_fmt_pack_floats() = DINER_FMT_PACK_FLOATS floats, 16-byte aligned: the matrices of one encoder layer TRANSPOSED
 * ([in][out], element [k][j] = weight[j][k] of the torch Linear) in the order query, key, value, out projection (32 x 32 each), linear1
 * (32 x 64), linear2 (64 x 32), then the vectors query, key, value, out bias, norm1 weight, norm1 bias, linear1 bias (64), linear2 bias,
 * norm2 weight, norm2 bias.
 *
 * diner_fmt_tokenise_f32: tokens[n][y W + x][c] = x[n][c][y][x] + pe[c][y][x], x (N,C,H,W) NCHW with C = 32, pe (C,pe_h,pe_w) the sine
 *   positional encoding of which the top-left H x W is read; one fp32 add.
 * diner_fmt_kv_f32: the attention state of the source tokens src (N,L,32) under the pack's key and value projections:
 *   K = elu(src Wk^T + bk) + 1, V = src Wv^T + bv (each the bias plus one fmaf chain, k ascending); per head h of 4 channels
 *   KV[h][m][d] = sum_s K[s][4 h + d] V[s][4 h + m], Ksum[h][d] = sum_s K[s][4 h + d]; state (N, DINER_FMT_STATE_FLOATS): KV as
 *   [h][m][d] (128 floats), then Ksum [h][d] (32).  Workgroup b of an image sums tokens [b T, (b + 1) T), T = DINER_FMT_KV_TOKENS, in double
 *   (the 64 lanes' xor tree, then the four waves in order) into partials (N, diner_fmt_kv_blocks(L), 160) doubles, workspace; a second
 *   launch adds an image's partials in block order and rounds once to float.
 * diner_fmt_layer_f32: one encoder layer per token, out (N,L,32) (may be x): Q = elu(x Wq^T + bq) + 1; per head Z = 1 / (Q . Ksum + 1e-6),
 *   A[m] = Z sum_d Q[d] KV[m][d]; x1 = LN1(x + A Wo^T + bo); y = relu(x1 W1^T + b1) W2^T + b2; out = LN2(x1 + y); LayerNorm over the 32
 *   channels with the biased variance, eps 1e-5, affine.  Image n reads row n mod state_rows of state (state_rows, 160): state_rows = N
 *   for a self layer, = the batch size for a cross layer whose images are ordered view-major (n = view B + b).  state_rows divides N.
 * diner_fpn_merge_f32: y (N,2H,2W,Clat) = bilinear2x(conv1x1(top)) + lateral: top (N,H,W,Ctop), w (Clat,Ctop) the bias-free 1 x 1
 *   convolution, computed at the coarse size into reduced (N,H,W,Clat), workspace; the upsampling is
 *   F.interpolate(mode="bilinear", align_corners=False) at exactly twice the size (phases 0.25 / 0.75, the edge clamped), evaluated as
 *   ly0 (lx0 p00 + lx1 p01) + ly1 (lx0 p10 + lx1 p11).  Ctop <= DINER_FPN_MAX_CHANNELS, Clat a multiple of 4 up to it; two launches. */
#define DINER_FMT_D_MODEL 32
#define DINER_FMT_NHEAD 8
#define DINER_FMT_D_FF 64
#define DINER_FMT_MAX_HW 600
#define DINER_FMT_STATE_FLOATS 160
#define DINER_FMT_KV_TOKENS 512
#define DINER_FMT_PACK_FLOATS 8544
#define DINER_FPN_MAX_CHANNELS 64
size_t diner_fmt_pack_floats(void);
size_t diner_fmt_kv_blocks(int L);
int diner_fmt_tokenise_f32(const float* x, const float* pe, float* tokens, int N, int C, int H, int W, int pe_h, int pe_w, void* stream);
int diner_fmt_kv_f32(const float* src, const float* pack, double* partials, float* state, int N, int L, void* stream);
int diner_fmt_layer_f32(const float* x, const float* pack, const float* state, float* out, int N, int L, int state_rows, void* stream);
int diner_fpn_merge_f32(const float* top, const float* w, const float* lateral, float* reduced, float* y, int N, int H, int W, int Ctop,
                        int Clat, void* stream);

/* ---- the depth estimator's FeatureNet (csrc/deform.hip, csrc/conv2d.hip) ---------------------------------------------------------------
 * What TransMVSNet's FeatureNet (models/module.py:343-421) needs beyond diner_conv3x3_f32 and diner_encoder_input_f32 (pad 0, C 4).
 * Activations are channels-last fp32 (N,H,W,C); every function refuses bad arguments with DINER_E_INVALID and a message before any
 * device work; every output is computed in an order the shape alone fixes (no atomics), a tile never crosses images, so an image's
 * values are the same bits at any batch position.  A BatchNorm that follows a layer is folded into its weights and bias by the caller.
 *
 * diner_deform_conv3x3_f32: torchvision's modulated deform_conv2d, 3 x 3, stride 1, padding 1, dilation 1, one offset group:
 *   offmask (N,H,W,27), the raw output of the layer's conv_offset_mask: for tap k = 3 ky + kx, dy_k = offmask[2 k], dx_k = offmask[2 k + 1],
 *   m_k = sigmoid(offmask[18 + k]);
 *     y[n,h,w,o] = bias[o] + sum_k sum_c w[o,c,ky,kx] m_k S(x[n,:,:,c], h - 1 + ky + dy_k, w - 1 + kx + dx_k)   [then ReLU if relu]
 *   S(., py, px) is torchvision's bilinear_interpolate in fp32: 0 when py <= -1, py >= H, px <= -1 or px >= W (or either is NaN);
 *   otherwise y0 = floor(py), ly = py - y0, hy = 1 - ly (columns likewise), a corner outside the image contributes 0, and the value is
 *   ((hy hx v00 + hy lx v01) + ly hx v10) + ly lx v11, every product and sum rounded.  Offsets may be any float: +-1e30, +-inf and NaN
 *   are plain "outside" and no address is formed from them.  The sampled matrix never reaches global memory.
 *   K order of an output: the bias, then taps k = 0 .. 8 ascending, within a tap channels c = 0 .. Cin - 1 ascending, one fmaf chain
 *   (v_mfma_f32_16x16x4_f32).  Cin a multiple of 8 in [8, DINER_DEFORM_MAX_CIN]; any Cout >= 1; H, W <= 2^14; N <= 65535.
 *   wpack: diner_deform_conv3x3_pack_floats(Cin, Cout) floats (0 for arguments the function refuses), 16-byte aligned,
 *   [ceil(Cout / BN)][k][Cin][BN] with BN = 16 for Cout <= 16, else 32; element [t][k][c][j] = w[BN t + j][c][k / 3][k % 3], zeros beyond
 *   Cout.  bias: Cout floats or NULL.  x 16-byte aligned; y must not be x or offmask.
 * diner_conv5x5_s2_f32 / diner_conv1x1_f32: y = conv(x, w) + bias [then ReLU], 5 x 5 stride 2 zero padding 2 (Ho = (H - 1) / 2 + 1) and
 *   1 x 1 stride 1, any Cin, Cout >= 1, N <= 65535, on diner_conv3x3_f32's kernel and in its K order (chunk of 8 channels, kernel row,
 *   kernel column, channel).  wpack: diner_conv5x5_s2_pack_floats / diner_conv1x1_pack_floats floats, 16-byte aligned,
 *   [ceil(Cin / 8)][ky R + kx][8][Cout rounded up to 64].  bias: Cout floats or NULL.  (diner_conv2d_s2_f32 itself keeps refusing R = 5.)
 * diner_fpn_lateral_f32: y (N,H,W,Ctop) = top[n, h / 2, w / 2, :] + (bias + w lateral[n,h,w,:]): the pyramid's nearest 2 x upsampling
 *   of top (N,H/2,W/2,Ctop) plus the 1 x 1 convolution w (Ctop,Clat), bias (Ctop or NULL) of lateral (N,H,W,Clat), one launch and no
 *   intermediate; the convolution is one fmaf chain from the bias, k ascending, the coarse pixel is added last.  H, W even; Ctop a
 *   multiple of 4 up to DINER_FPN_MAX_CHANNELS, Clat up to it; top and y 16-byte aligned; y must not be an input. */
#define DINER_DEFORM_MAX_CIN 64
size_t diner_deform_conv3x3_pack_floats(int Cin, int Cout);
int diner_deform_conv3x3_f32(const float* x, const float* offmask, const float* wpack, const float* bias, float* y, int N, int H, int W,
                             int Cin, int Cout, int relu, void* stream);
size_t diner_conv5x5_s2_pack_floats(int Cin, int Cout);
int diner_conv5x5_s2_f32(const float* x, const float* wpack, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int relu,
                         void* stream);
size_t diner_conv1x1_pack_floats(int Cin, int Cout);
int diner_conv1x1_f32(const float* x, const float* wpack, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int relu,
                      void* stream);
int diner_fpn_lateral_f32(const float* top, const float* lateral, const float* w, const float* bias, float* y, int N, int H, int W, int Ctop,
                          int Clat, void* stream);

/* ---- the deformable convolution's gradients (csrc/deform_grad.hip) -----------------------------------------------------------------------
 * New symbols without an ABI bump.  diner_deform_conv3x3_grad_f32: the backward pass of diner_deform_conv3x3_f32 with relu = 0, from the
 * upstream gradient dy (N,H,W,Cout), channels-last fp32 like x (N,H,W,Cin) and the raw offmask (N,H,W,27); weight is the plain
 * (Cout,Cin,3,3) tensor, not the forward's packed one.  With m = sigmoid(offmask[18 + k]), S the forward's sample, v00 .. v11 its corner
 * values (0 where a corner is not valid) and G[p,k,c] = sum_o dy[p,o] w[o,c,k]:
 *   d_offmask[p,18 + k] = m (1 - m) sum_c G S                                     (the sigmoid's derivative included)
 *   d_offmask[p,2 k]    = m sum_c G (-hx v00 - lx v01 + hx v10 + lx v11)          d_offmask[p,2 k + 1] = m sum_c G (-hy v00 + hy v01 - ly v10 + ly v11)
 *   d_x[corner i, c]   += m wt_i G[p,k,c]     d_weight[o,c,k] = sum_p dy[p,o] m S     d_bias[o] = sum_p dy[p,o]
 * torchvision's rule, and autograd's through the floor: at an exactly integer coordinate the right-sided difference.  A tap whose offset
 * puts it outside (NaN, +-inf, +-1e30 included) reads nothing and every gradient of it is exactly 0.
 *   Outputs: d_x (N,H,W,Cin), d_offmask (N,H,W,27), d_weight (Cout,Cin,3,3), d_bias (Cout); each may be NULL ("not wanted": its work is
 *   skipped, the others' bits do not change).  d_offmask, d_weight and d_bias are written once per element in an order the shape (and
 *   `slabs`) alone fixes: the same bits on every run, d_offmask also at any batch position.  d_x is zeroed with hipMemsetAsync and then
 *   added to with native float atomics, whose order is free: d_x IS NOT BIT-REPRODUCIBLE from run to run.
 *   workspace: diner_deform_conv3x3_grad_workspace_floats(N, H, W, Cin, Cout, slabs) floats (0 for arguments the function refuses), needed
 *   for d_weight or d_bias: S slabs of per-workgroup sums, which a finish launch adds in slab order in double, rounded once.  slabs: 0
 *   for the default S = min(tiles, 128) with tiles = N ceil(H W / 64); a positive value forces S = min(slabs, tiles, 1024).
 *   Limits, refused with DINER_E_INVALID before any device work: Cin a multiple of 8 in [8, DINER_DEFORM_MAX_CIN]; Cout in
 *   [1, DINER_DEFORM_MAX_CIN]; H, W <= 2^14; N <= 65535; fewer than 2^30 tiles; x 16-byte aligned; d_x and d_offmask none of the inputs. */
size_t diner_deform_conv3x3_grad_workspace_floats(int N, int H, int W, int Cin, int Cout, int slabs);
int diner_deform_conv3x3_grad_f32(const float* x, const float* offmask, const float* weight, const float* dy, float* d_x, float* d_offmask,
                                  float* d_weight, float* d_bias, float* workspace, int N, int H, int W, int Cin, int Cout, int slabs,
                                  void* stream);

/* ---- the feature transformer's gradients (csrc/fmt_grad.hip) ----------------------------------------------------------------------------
 * New symbols without an ABI bump.  diner_fmt_layer_grad_f32: the backward pass of one encoder layer, diner_fmt_kv_f32 on `source`
 * (R,S,32) followed by diner_fmt_layer_f32 on x (N,L,32) with state_rows = R, from the upstream gradient dy (N,L,32).  pack and state
 * are the forward's; nothing else is saved from the forward, the kernels compute it again with the forward's own fmaf chains.  With
 * Q = elu(x Wq^T + bq) + 1, den_h = Q_h . Ksum_h + 1e-6, A = (Q KV) / den and dA the gradient at A:
 *   d_state[r]: dKV[h][m][d] = sum dA[h][m] Q[h][d] / den_h, dKsum[h][d] = sum -(sum_m dA[h][m] A[h][m]) Q[h][d] / den_h over the tokens of
 *     every image n with n mod R = r; products and sums in double, in (image, tile) order, rounded once.  It stays in the workspace.
 *   d_source: dK = dKV V + dKsum, dV = dKV^T K, dkp = dK elu'(kp), d_source = dkp Wk + dV Wv.
 *   d_x: through LN2, the feed-forward (relu'(0) = 0), LN1, the out projection, the query side and both residuals.
 *   d_params, DINER_FMT_PACK_FLOATS floats: the sixteen parameter gradients in the pack's order with the matrices as torch keeps them,
 *     (out, in): Wq Wk Wv Wo W1 W2, then bq bk bv bo g1 be1 b1 b2 g2 be2.
 *   Each of d_x, d_source, d_params may be NULL ("not wanted": its work is skipped, the others' bits do not change).  accumulate != 0
 *   is the self layer: source must be x, R = N, S = L, d_source NULL, and d_x receives the sum of both paths.
 *   A tile is DINER_FMT_GRAD_TOKENS tokens of one image, one thread a token.  A workgroup walks ceil(tiles / slabs) consecutive tiles and
 *   keeps one slab of parameter sums (DINER_FMT_GRAD_QUERY_SLAB_FLOATS on the query side, DINER_FMT_GRAD_SOURCE_SLAB_FLOATS on the source
 *   side): a tile's sum is one fmaf chain from 0 in token order, the slab adds its tiles in order as a (sum, carry) pair of floats; a
 *   finish launch adds the slabs with their carries in slab order in double and rounds once.  slabs: 0 for
 *   min(tiles, 128) on either side, or a count up to DINER_FMT_GRAD_MAX_SLABS.  No atomics: every output has the same bits on every run,
 *   and an image's d_x does not depend on its place in the batch.
 *   workspace: diner_fmt_layer_grad_workspace_floats(N, L, R, S, slabs) floats (0 for arguments the function refuses), 16-byte aligned;
 *   needed unless only d_x of a cross layer is asked for.
 *   Limits, refused with DINER_E_INVALID before any device work: N <= 65535; R a divisor of N; L, S in [1, DINER_FMT_MAX_HW^2]; the
 *   tokens, the pack and the token gradients 16-byte aligned; d_x and d_source none of the inputs. */
#define DINER_FMT_GRAD_TOKENS 128
#define DINER_FMT_GRAD_QUERY_SLAB_FLOATS 6432
#define DINER_FMT_GRAD_SOURCE_SLAB_FLOATS 2112
#define DINER_FMT_GRAD_MAX_SLABS 1024
size_t diner_fmt_layer_grad_workspace_floats(int N, int L, int R, int S, int slabs);
int diner_fmt_layer_grad_f32(const float* x, const float* source, const float* pack, const float* state, const float* dy, int N, int L, int R,
                             int S, float* d_x, float* d_source, float* d_params, float* workspace, int accumulate, int slabs, void* stream);

/* ---- the depth estimator's fine-tuning objective and depth scores ------------------------------------------------------------------------
 * New symbols without an ABI bump (mvsloss.hip): TransMVSNet's entropy_loss / focal_loss_bld / trans_mvsnet_loss (models/module.py:490-587)
 * with the gradient, and Thres_metrics / AbsDepthError_metrics (utils.py:240-274).  No allocation, enqueue-only, no host read-back, no
 * atomics.  A workgroup (256 pixels) belongs to one image and writes DINER_MVS_LOSS_SLOTS doubles to its own slot of `partials`
 * (diner_mvs_loss_partial_doubles(B, H, W) doubles); an image's slots are added in an order the shape alone fixes, so two runs give the
 * same bits and an image's sums, depth and gradient do not depend on its place in the batch (the 1 / B of the gradient is the same number
 * everywhere).  Limits, refused with DINER_E_INVALID before any device work: B, D, H, W >= 1 and B D H W < 2^31.
 *
 * diner_mvs_stage_loss_f32: one stage's forward.  Exactly one of cost (B,D,H,W; init, the reference's prob_volume_init, is added first
 *   when non-NULL) and prob (B,D,H,W, already a probability volume) is non-NULL.  hypotheses (B,D,H,W), gt (B,H,W), mask (B,H,W) float,
 *   valid where > 0.5.  Per pixel, one thread, diner_mvs_select_depth_f32's operation chain: prob = exp(log_softmax(cost [+ init]));
 *   g = the first index of min_d |hyp_d - gt| in fp32, 0 where the mask is off; ce = -logf(prob[g] + 1e-6f); depth (B,H,W) =
 *   hyp[first argmax prob] and confidence (B,H,W) = max prob (the bits of diner_mvs_select_depth_f32); err = |depth - gt| and
 *   smooth_l1(err), beta 1, in double.  record (B,H,W,4 floats, 16-byte aligned) when non-NULL: g (int bits), prob[g], the softmax's
 *   maximum and log-sum -- what the gradient needs.  Partial sums per workgroup: valid, sum ce, sum smooth-L1, sum err, and, when
 *   unit (B doubles: the scores' error unit per image, the reference's depth_interval 192 / 128) is non-NULL, sum err / unit and the counts
 *   of err / unit < thresholds[t] (n_thresholds <= DINER_MVS_LOSS_MAX_THRESHOLDS host doubles).  A pixel whose mask is off adds exactly
 *   nothing, whatever gt holds there (NaN, inf).
 * diner_mvs_loss_finish_f32: one wave adds the per-image sums -> scalars (DINER_MVS_LOSS_SCALARS floats, each a double rounded once):
 *   [0] weight 2 entropy, [1] 2 entropy with entropy = mean_b(sum_b ce / v_b), v_b = float32(valid_b) + 1e-6 rounded to float32 as the
 *   reference's valid_pixel_num is (an image without a valid pixel adds 0),
 *   [2] depth_loss = sum smooth-L1 / sum valid over the batch (NaN when nothing is valid), [3] sum err / sum valid, [4] sum (err / unit) /
 *   sum valid, [5 + t] the share of valid pixels with err / unit < thresholds[t]; factors (B doubles) = 1 / (B v_b);
 *   sums (B, DINER_MVS_LOSS_SLOTS doubles): the per-image sums in the slot order above, zeros beyond.
 * diner_mvs_stage_loss_grad_f32: grad (B,D,H,W), every element written, = d(upstream weight 2 entropy) / d(cost) -- with
 *   G = -upstream weight 2 factors[b] / (p_g + 1e-6), grad_j = G p_g ((j == g) - p_j), p_j recomputed from the record's maximum and
 *   log-sum -- or, with from_prob, / d(prob): G at plane g, zero elsewhere (cost may then be NULL).  upstream: one float on the device.
 *   Pixels whose mask is off get zeros.
 * diner_depth_scores_f32: est, gt, mask (B,H,W) -> per_image (B, DINER_DEPTH_SCORES floats): over the image's valid pixels the mean of
 *   err = |est - gt| (NaN without one), the mean of the errs inside [band_lo, band_hi] when has_band (0 when none is inside), and per
 *   threshold t the share of errs > thresholds[t]; batch (DINER_DEPTH_SCORES floats): the mean of the per-image values, images in order,
 *   as the reference's compute_metrics_for_each_image.  The same double sums; partials as above. */
#define DINER_MVS_LOSS_SLOTS 16
#define DINER_MVS_LOSS_MAX_THRESHOLDS 8
#define DINER_MVS_LOSS_SCALARS 13
#define DINER_DEPTH_SCORES 10
size_t diner_mvs_loss_partial_doubles(int B, int H, int W);
int diner_mvs_stage_loss_f32(const float* cost, const float* init, const float* prob, const float* hypotheses, const float* gt,
                             const float* mask, const double* unit, const double* thresholds, int n_thresholds, float* depth,
                             float* confidence, float* record, double* partials, int B, int D, int H, int W, void* stream);
int diner_mvs_loss_finish_f32(const double* partials, int B, int H, int W, int n_thresholds, double weight, float* scalars, double* factors,
                              double* sums, void* stream);
int diner_mvs_stage_loss_grad_f32(const float* cost, const float* init, int from_prob, const float* mask, const float* record,
                                  const double* factors, const float* upstream, double weight, float* grad, int B, int D, int H, int W,
                                  void* stream);
int diner_depth_scores_f32(const float* est, const float* gt, const float* mask, int B, int H, int W, const double* thresholds,
                           int n_thresholds, int has_band, double band_lo, double band_hi, double* partials, float* per_image, float* batch,
                           void* stream);

/* ---- measurement aid (bench.py): per-kernel durations of the two field kernels ------------------
 * With profiling enabled every field call brackets k_field_pre / k_field_post with HIP events on the
 * launch stream; diner_profile_collect waits for them, returns the summed durations (ms), the number
 * of launches of each kernel and the points they processed, and resets the log. */
int diner_profile_enable(int enable);
int diner_profile_collect(double* pre_ms, double* post_ms, long long* launches, long long* points);

#ifdef __cplusplus
}
#endif
#endif /* DINER_HIP_H */
