// The one-launch form of the ray chunk (K1..K5 in one kernel, no conditioning rows in HBM): decoder_kernel<4,SP,2,CVF = 1> of
// decoder_staged.hpp, whose workgroups first produce their tile's conditioning rows with the cost-volume walk of cv_walk.hpp,
// and the two functions mnerf_render_chunk (render_chunk.hip) reaches it through.  An object of its own, so that the library
// holds each kernel once.  Those workgroups run the walk on SIMDs where another workgroup issues 16-bit 32x32x16 matrix
// instructions: see "packed fp32 next to 16-bit MFMA" in DESIGN.md (section 4) - what round 2 recorded as an unexplained race of
// co-resident fused workgroups - and the flags of this file in build.py.
#include "decoder_staged.hpp"

// The fused ray-chunk form (one launch, no workspace) exists for the shipped configuration class: split-fp16
// stream, S <= 128, at most 32 conditioning inputs (<= 5 views), cosine groups of at most 8 lanes (G >= 2) and
// walk scratch that fits one weight buffer.
bool mnerf_fused_render_applies(const mnerf_scene* sc, const mnerf_decoder* dec, const mnerf_rays* rays) {
  if (dec->wstream_format != MNERF_WSTREAM_F16X2 || rays->n_samples > 128) return false;
  if (rays->pose_table) return false;  // pose tables: two-launch form only
  if (dec->cond_stride > 32 || (dec->cond_dim + 15) / 16 > 2) return false;
  if (sc->n_views < 2 || sc->n_views != dec->n_views) return false;
  int sumG = 0;
  for (int s = 0; s < sc->n_scales; ++s) {
    if (sc->n_group[s] < 2) return false;
    sumG += sc->n_group[s];
  }
  if (sumG > 16) return false;
  return 16 * cv_slot_lds_floats(CVF_SEG, sc->n_views, sumG) <= SEG_CAP_FLOATS &&
         CVF_COND_OFF_FLOATS + 128 * dec->cond_stride <= SEG_CAP_FLOATS;
}

int mnerf_fused_render_launch(const mnerf_scene* sc, const mnerf_decoder* dec, const mnerf_rays* rays, float* rgb,
                              float* depth, float* opacity, void* stream) {
  float *rgb_s = nullptr, *sigma = nullptr;
#ifdef MNERF_FUSED_DEBUG
  if (const char* e = getenv("MNERF_FDBG_RGBS")) rgb_s = (float*)strtoull(e, nullptr, 0);
  if (const char* e = getenv("MNERF_FDBG_SIGMA")) sigma = (float*)strtoull(e, nullptr, 0);
#endif
  const DecCall c = {"mnerf_render_chunk", dec, &sc->views[0], rays, nullptr, rgb, depth, opacity, rgb_s, sigma,
                     nullptr, nullptr, sc, stream};
  int Sp;
  DecSched sch;
  if (const int err = check_decoder_call(c, &Sp, &sch)) return err;
  if (rays->n_rays == 0) return MNERF_OK;
  return launch_staged<1>(c, sch, Sp);
}
