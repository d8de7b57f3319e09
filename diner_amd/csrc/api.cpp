// Host-side plumbing shared by all entry points of libdiner_hip.so.
#include <stdarg.h>
#include "common.hpp"

namespace diner {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_fused_views(int nv, const char* who) {
  DINER_CHECK_ARG(nv >= 1 && nv <= kMaxViewsWide, "%s: nv=%d outside [1,%d]", who, nv, kMaxViewsWide);
  if (nv > kMaxViews) {
    set_error("%s: nv=%d source views -- this entry is built for at most %d (the 4-view limit of the fused kernels); scenes with up to "
              "%d views render, sample and train on the generic exact-fp32 path", who, nv, kMaxViews, kMaxViewsWide);
    return DINER_E_UNSUPPORTED;
  }
  return 0;
}

template <int NMAX>
static int fill_scene_dev(const DinerScene* s, SceneDevT<NMAX>* out) {
  DINER_CHECK_ARG(s->poses_host && s->focal_host && s->c_host, "scene: poses_host/focal_host/c_host (host arrays) missing");
  DINER_CHECK_ARG(s->img_w > 0 && s->img_h > 0, "scene: image_shape must be positive");
  memset(out, 0, sizeof(*out));
  out->latent_cl = s->latent_cl;
  out->depth = s->depth;
  out->depth_std = s->depth_std;
  out->normals = s->normals;
  out->std_pad_scale = s->std_pad_scale;
  for (int v = 0; v < s->nv; ++v) {
    const float* P = s->poses_host + 16 * v;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) out->R[v][3 * i + j] = P[4 * i + j];
      out->t[v][i] = P[4 * i + 3];
    }
    out->focal[v][0] = s->focal_host[2 * v];
    out->focal[v][1] = s->focal_host[2 * v + 1];
    out->c[v][0] = s->c_host[2 * v];
    out->c[v][1] = s->c_host[2 * v + 1];
  }
  out->img_w = s->img_w;
  out->img_h = s->img_h;
  out->feature_padding = s->feature_padding;
  out->nv = s->nv;
  out->C = s->C;
  out->Hf = s->Hf;
  out->Wf = s->Wf;
  out->Hs = s->Hs;
  out->Ws = s->Ws;
  return 0;
}

int make_scene_dev(const DinerScene* s, SceneDev* out) {
  DINER_CHECK_ARG(s != nullptr, "scene is null");
  int rc = check_fused_views(s->nv, "scene");
  if (rc) return rc;
  return fill_scene_dev(s, out);
}

int make_scene_dev(const DinerScene* s, SceneDevWide* out) {
  DINER_CHECK_ARG(s != nullptr, "scene is null");
  DINER_CHECK_ARG(s->nv >= 1 && s->nv <= kMaxViewsWide, "scene: nv=%d outside [1,%d]", s->nv, kMaxViewsWide);
  return fill_scene_dev(s, out);
}

int make_group_scene_dev(const DinerScene* s, int g, SceneDev* out, int* n_live) {
  DINER_CHECK_ARG(s != nullptr && s->nv >= 1 && s->nv <= kMaxViewsWide, "scene: nv outside [1,%d]", kMaxViewsWide);
  const int v0 = kMaxViews * g;
  DINER_CHECK_ARG(g >= 0 && v0 < s->nv, "scene: view group %d of a scene with %d views", g, s->nv);
  const int live = s->nv - v0 < kMaxViews ? s->nv - v0 : kMaxViews;
  DinerScene grp = *s;
  grp.nv = live;
  grp.poses_host = s->poses_host + 16 * v0;
  grp.focal_host = s->focal_host + 2 * v0;
  grp.c_host = s->c_host + 2 * v0;
  const size_t hw_f = (size_t)s->Hf * s->Wf, hw_s = (size_t)s->Hs * s->Ws;
  if (s->latent_cl) grp.latent_cl = s->latent_cl + (size_t)v0 * hw_f * s->C;
  if (s->depth) grp.depth = s->depth + (size_t)v0 * hw_s;
  if (s->depth_std) grp.depth_std = s->depth_std + (size_t)v0 * hw_s;
  if (s->normals) grp.normals = s->normals + (size_t)v0 * 3 * hw_s;
  int rc = fill_scene_dev(&grp, out);
  if (rc) return rc;
  for (int v = live; v < kMaxViews; ++v) {      // dead columns: the group's first camera
    memcpy(out->R[v], out->R[0], sizeof(out->R[0]));
    memcpy(out->t[v], out->t[0], sizeof(out->t[0]));
    memcpy(out->focal[v], out->focal[0], sizeof(out->focal[0]));
    memcpy(out->c[v], out->c[0], sizeof(out->c[0]));
  }
  *n_live = live;
  return 0;
}

int check_mlp_config(const DinerMlpParams* p, const char* who, bool poscode) {
  DINER_CHECK_ARG(p && p->lin_in_w && p->lin_in_b && p->lin_out_w && p->lin_out_b && p->fc0_w && p->fc0_b && p->fc1_w &&
                      p->fc1_b && p->lin_z_w && p->lin_z_b, "%s: parameter pointers missing", who);
  if (p->d_in != 55 || p->d_latent != 512 || p->d_hidden != 512 || p->d_out != 4 || p->n_blocks != 5 ||
      p->combine_layer != 3) {
    set_error("%s: unsupported ResnetFC configuration d_in=%d d_latent=%d d_hidden=%d d_out=%d n_blocks=%d "
              "combine_layer=%d (built for 55/512/512/4/5/3, configs/train_dtu.yaml:44-50)",
              who, p->d_in, p->d_latent, p->d_hidden, p->d_out, p->n_blocks, p->combine_layer);
    return DINER_E_UNSUPPORTED;
  }
  if (poscode) {
    // d_in = 3 * (2 F + 1) + (2 F + 1) + 3 = 55 fixes F = 6 with the input included (pixelnerf.py:15-18)
    if (p->num_freqs != 6 || !p->include_input) {
      set_error("%s: unsupported positional encoding num_freqs=%d include_input=%d (built for 6 / 1, "
                "configs/train_dtu.yaml:39-43)", who, p->num_freqs, p->include_input);
      return DINER_E_UNSUPPORTED;
    }
    // the in-kernel sine is accurate for arguments below ~2^13: |x_c| * freq_factor * 32 with |x_c| up to a few units
    if (!(p->freq_factor > 0.0f && p->freq_factor <= 64.0f)) {
      set_error("%s: unsupported positional encoding freq_factor=%g (supported: (0, 64]; 6.28 in the shipped configs)",
                who, (double)p->freq_factor);
      return DINER_E_UNSUPPORTED;
    }
  }
  return 0;
}

}  // namespace diner

extern "C" int diner_abi_version(void) { return DINER_ABI_VERSION; }
extern "C" const char* diner_last_error(void) { return diner::g_err; }
