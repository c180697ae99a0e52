// libmnerf_hip.so — error channel and ABI version (see include/mnerf.h).
#include <string.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>

#include "common.hpp"
#include "launch_plan.hpp"

static thread_local char g_err[512] = "";

void mnerf_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int mnerf_abi_version(void) { return MNERF_ABI_VERSION; }
extern "C" const char* mnerf_last_error(void) { return g_err; }

// sizeof() of the by-value argument structs as compiled into the library, so that a binding
// in another language can verify its own struct mirrors (0 view, 1 rays, 2 scene, 3 decoder).
extern "C" int64_t mnerf_struct_size(int32_t which) {
  switch (which) {
    case 0: return (int64_t)sizeof(mnerf_view);
    case 1: return (int64_t)sizeof(mnerf_rays);
    case 2: return (int64_t)sizeof(mnerf_scene);
    case 3: return (int64_t)sizeof(mnerf_decoder);
    case 4: return (int64_t)sizeof(mnerf_encoder_layer);
    case 5: return (int64_t)sizeof(mnerf_conv);
    case 6: return (int64_t)sizeof(mnerf_decoder_train);
    case 7: return (int64_t)sizeof(mnerf_encoder_layer_train);
    case 8: return (int64_t)sizeof(mnerf_optim_row);
    case 9: return (int64_t)sizeof(mnerf_optim_group);
    case 10: return (int64_t)sizeof(mnerf_lpips_weights);
    case MNERF_STRUCT_CAMERA: return (int64_t)sizeof(mnerf_camera);
    default: return -1;
  }
}

int mnerf_rays_canonical(const mnerf_rays* rays, mnerf_rays* out, const char* who) {
  MNERF_REQUIRE(rays, MNERF_E_NULL, "%s: rays is NULL", who);
  *out = *rays;
  MNERF_REQUIRE(rays->tgt_height >= 0 && rays->tgt_width >= 0 && (rays->tgt_height == 0) == (rays->tgt_width == 0), MNERF_E_RANGE,
                "%s: target grid %dx%d (both 0 = the views' size, or both >= 1)", who, rays->tgt_height, rays->tgt_width);
  if (rays->tgt_height == 0) out->tgt_height = rays->height, out->tgt_width = rays->width;
  MNERF_REQUIRE(out->tgt_height >= 1 && out->tgt_width >= 1, MNERF_E_RANGE, "%s: target grid %dx%d", who, out->tgt_height,
                out->tgt_width);
  if (!rays->ray_idx && !rays->pose_table && rays->n_rays > 0)
    MNERF_REQUIRE(rays->ray_begin >= 0 && (long long)rays->ray_begin + rays->n_rays <= (long long)out->tgt_height * out->tgt_width,
                  MNERF_E_RANGE, "%s: pixels [%d, %d + %d) outside the %dx%d target grid", who, rays->ray_begin, rays->ray_begin,
                  rays->n_rays, out->tgt_height, out->tgt_width);
  return MNERF_OK;
}

int mnerf_free_rays_canonical(const mnerf_rays* rays, const float* ray_od, mnerf_rays* out, const char* who) {
  MNERF_REQUIRE(rays, MNERF_E_NULL, "%s: rays is NULL", who);
  MNERF_REQUIRE(!rays->ray_idx && !rays->pose_table, MNERF_E_UNSUPPORTED,
                "%s: a ray bundle excludes ray_idx / pose_table (the bundle's rows are the rays)", who);
  MNERF_REQUIRE(rays->n_rays >= 0 && rays->n_samples >= 1, MNERF_E_RANGE, "%s: n_rays=%d S=%d", who, rays->n_rays, rays->n_samples);
  MNERF_REQUIRE(rays->legacy_coord == 0 || rays->n_samples >= 2, MNERF_E_RANGE, "%s: legacy depth sampling needs S >= 2", who);
  if (rays->n_rays > 0) {
    MNERF_REQUIRE(ray_od, MNERF_E_NULL, "%s: ray_od is NULL", who);
    MNERF_REQUIRE(mnerf_aligned16(ray_od), MNERF_E_ALIGN, "%s: ray_od not 16B aligned", who);
  }
  mnerf_rays c = {};
  c.n_rays = rays->n_rays, c.n_samples = rays->n_samples;
  c.legacy_coord = rays->legacy_coord ? 1 : 0, c.depth_inverse = rays->depth_inverse ? 1 : 0;
  c.height = c.tgt_height = rays->height, c.width = c.tgt_width = rays->width;
  c.near_ = rays->near_, c.far_ = rays->far_;
  c.strat_u = rays->strat_u;
  *out = c;
  return MNERF_OK;
}

// ---- debug / tuning knobs: the environment is read ONCE, when the library is loaded (a static initialiser), into a
// table that launches only read (mnerf_debug_set_knob below is the one writer, for tests).  Nothing in a launch path calls getenv or keeps mutable state; the only
// per-process bookkeeping left is "has this kernel's LDS attribute been set on this device" (mnerf_once_per_device).
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return (e && *e) ? atoi(e) : dflt;
}

static mnerf_tuning read_tuning() {
  mnerf_tuning t;
  t.decoder_grid = env_int("MNERF_DECODER_GRID", 512);          // persistent: 2 workgroups per CU x 256 CUs
  t.decoder_stagger = env_int("MNERF_DECODER_STAGGER", 16);     // ~130k cycles ~ half a tile
  t.decoder_stagger_mode = env_int("MNERF_DECODER_STAGGER_MODE", 0);
  t.cv_variant = env_int("MNERF_CV_VARIANT", 3);  // 3 / 4 = segment walk with 16 / 8 lanes per sample; 5 = texel tiles in LDS (slower, kept: cost_volume.hip); 0 = plain
  t.cv_mm = env_int("MNERF_CV_MM", 1);            // matrix form of the cost volume where it applies (cost_volume_mm.hip)
  t.cv_mm_spw = env_int("MNERF_CV_MM_SPW", 4);
  t.cv_uvpair = env_int("MNERF_CV_UVPAIR", -1);
  t.cv_pair_block = env_int("MNERF_CV_PAIR_BLOCK", -1);
  t.cv_grid = env_int("MNERF_CV_GRID", 0);        // 0 = the variant's default cap
  t.wa_min4 = env_int("MNERF_WA_MIN4", 200);      // 128-query workgroups once they (nearly) fill the 256 CUs
  t.wa_xcd = env_int("MNERF_WA_XCD", 1);          // query blocks of a window share an XCD (its L2 holds the K / V images)
  t.render_fused = env_int("MNERF_RENDER_FUSED", 0);  // 1: mnerf_render_chunk takes the one-launch form where it applies
  t.decoder_pp = env_int("MNERF_DECODER_PP", 1);
  t.decoder_pp_grid = env_int("MNERF_DECODER_PP_GRID", 256);
  t.decoder_pp_max_s = env_int("MNERF_DECODER_PP_MAX_S", 256);
  return t;
}

// The table is read-only in production (filled from the environment at load).  The one writer is the test hook below; it and
// every reader go through g_tuning_lock, and a reader takes a COPY: a launch on another thread sees the table before or after a
// knob change, never a torn one (13 ints under an uncontended mutex per launch).
static mnerf_tuning g_tuning = read_tuning();
static std::mutex g_tuning_lock;
mnerf_tuning mnerf_tune() {
  std::lock_guard<std::mutex> hold(g_tuning_lock);
  return g_tuning;
}

// Test / diagnosis hook: change one knob of the table after load (what its environment variable would have set); the previous
// value comes back through *old_value, the return value is only the status.  Serialised with the launches' reads (above).
extern "C" int mnerf_debug_set_knob(const char* name, int value, int* old_value) {
  std::lock_guard<std::mutex> hold(g_tuning_lock);
  struct Knob { const char* name; int* slot; };
  const Knob knobs[] = {{"decoder_pp", &g_tuning.decoder_pp}, {"decoder_pp_grid", &g_tuning.decoder_pp_grid},
                        {"decoder_pp_max_s", &g_tuning.decoder_pp_max_s}, {"decoder_grid", &g_tuning.decoder_grid},
                        {"cv_variant", &g_tuning.cv_variant}, {"cv_mm", &g_tuning.cv_mm}, {"cv_mm_spw", &g_tuning.cv_mm_spw}, {"cv_uvpair", &g_tuning.cv_uvpair}, {"cv_pair_block", &g_tuning.cv_pair_block}, {"cv_grid", &g_tuning.cv_grid},
                        {"render_fused", &g_tuning.render_fused}, {"wa_min4", &g_tuning.wa_min4}};
  for (const Knob& k : knobs)
    if (name && strcmp(name, k.name) == 0) {
      if (old_value) *old_value = *k.slot;
      *k.slot = value;
      return MNERF_OK;
    }
  mnerf_set_error("mnerf_debug_set_knob: unknown knob '%s'", name ? name : "(null)");
  return MNERF_E_RANGE;
}

// Test / diagnosis hook: which kernel instance a launch of the given problem would take.  The rules live next to their launches
// (launch_plan.hpp lists them) and the launches call the same functions; nothing here touches the device.
extern "C" int mnerf_debug_launch_plan(const char* what, const int64_t* args, int32_t n_args, int32_t* plan, int32_t n_plan) {
  MNERF_REQUIRE(what && args && plan, MNERF_E_NULL, "mnerf_debug_launch_plan: NULL argument");
  struct Planner { const char* name; int (*fn)(const int64_t*, int32_t, int32_t*, int32_t); };
  const Planner planners[] = {{"conv2d", mnerf_plan_conv2d}, {"conv_gemm", mnerf_plan_conv_gemm}, {"conv_wgrad", mnerf_plan_conv_wgrad},
                              {"instance_norm", mnerf_plan_instance_norm}, {"instance_norm_backward", mnerf_plan_instance_norm},
                              {"window_attention", mnerf_plan_window_attention}};
  for (const Planner& p : planners)
    if (strcmp(what, p.name) == 0) return p.fn(args, n_args, plan, n_plan);
  mnerf_set_error("mnerf_debug_launch_plan: unknown dispatcher '%s'", what);
  return MNERF_E_RANGE;
}

bool mnerf_once_per_device(std::atomic<unsigned long long>& mask) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  return (mask.fetch_or(bit, std::memory_order_relaxed) & bit) == 0;
}
