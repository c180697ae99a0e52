/*
 * mnerf.h — C ABI of libmnerf_hip.so: the MI355X (gfx950) kernels of the MatchNeRF per-ray
 * rendering hot path.
 *
 * The reference (donydchen/matchnerf) is pure Python/PyTorch and has no FFI of its own
 * (SURVEY.md §8b): the seam is the Python class `MatchNeRF` (models/matchnerf.py:13-325).
 * This header is the boundary the build introduces *beneath* that class.  Each entry point
 * replaces one chain of eager PyTorch ops in the reference (file:line given per function).
 * The Python host (matchnerf_amd/hip.py) binds it with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain C: raw device pointers, explicit sizes, no torch / C++ types in any signature;
 *   - all tensors are fp32, row-major, contiguous unless a stride is given;
 *   - the caller allocates every buffer (inputs, outputs, scratch); functions only enqueue
 *     work on `stream` (a hipStream_t passed as void*; NULL = default stream): no
 *     allocation, no synchronisation => safe inside hipGraph capture;
 *   - small camera matrices travel BY VALUE inside the argument structs (kernel arguments),
 *     so no host->device copy is hidden in a call;
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *     MNERF_E_* argument-check code.  Nothing throws across the ABI.  The message of the
 *     last failure on the calling thread is available from mnerf_last_error();
 *   - launches go to the calling thread's CURRENT HIP device (hipSetDevice / torch.cuda.device):
 *     every pointer and the stream must belong to it;
 *   - process-wide state: none that a caller can observe.  Debug / tuning knobs (MNERF_DECODER_GRID,
 *     MNERF_DECODER_STAGGER[_MODE], MNERF_CV_VARIANT, MNERF_CV_GRID, MNERF_WA_MIN4, MNERF_WA_XCD, MNERF_RENDER_FUSED) are read from the
 *     environment ONCE, when the library is loaded; the library keeps one bit per (kernel, device) to
 *     remember that the kernel's dynamic-LDS attribute has been raised on that device.  The full list of knobs: INTEGRATION.md 4.
 *
 * ABI history (mnerf_abi_version(); struct sizes from mnerf_struct_size()):
 *   v6  mnerf_debug_set_knob returns the status and the previous value separately
 *   v7  mnerf_rays gained pose_table / rays_per_pose (several target poses per launch; mnerf_render_takes_pose_table).
 *       Added under v7 without a layout change: mnerf_debug_gemm, mnerf_window_attention_presplit_stats,
 *       mnerf_window_attention_backward_stats.
 *   v8  no layout change: mnerf_decoder.wstream_format accepts MNERF_WSTREAM_F16X1 (one-product fp16 fast mode); pose tables at
 *       sample_intvs <= 128 (was 64); mnerf_debug_set_knob serialised with the launches' reads.
 *   v9  mnerf_scene gained feat_op (appended: the offsets of the older fields are unchanged, sizeof grows by 8): the split-fp16
 *       OPERAND IMAGE of the feature maps that the matrix form of the cost volume reads (mnerf_cost_volume_operands,
 *       mnerf_cost_volume_operand_bytes).  NULL keeps the segment walk.
 *   v10 no layout change of the older structs: the tail of a training iteration (matchnerf_amd/csrc/optim.hip) - mnerf_optim_row
 *       and mnerf_optim_group - struct indices 8 and 9 -, mnerf_optim_row_blocks, mnerf_grad_sumsq, mnerf_adamw_step, mnerf_l2_loss.
 *   v11 no layout change: the gradient exchange of data-parallel training over the same row table - mnerf_grad_bucket_floats,
 *       mnerf_grad_pack, mnerf_grad_unpack.
 *   v12 no layout change: evaluation on the device (matchnerf_amd/csrc/metrics.hip) - mnerf_image_metrics,
 *       mnerf_image_metrics_workspace_bytes.
 *       Added under v12 without a layout change: LPIPS on the device (matchnerf_amd/csrc/lpips.hip) - the table mnerf_lpips_weights - struct
 *       index 10 -, mnerf_lpips_wstream_floats, mnerf_lpips_workspace_bytes, mnerf_lpips_vgg, mnerf_maxpool2x2, mnerf_lpips_head_slots,
 *       mnerf_lpips_head, mnerf_lpips_sum; mnerf_conv2d accepts c_out 256 / 512 (blocks of 128 output channels).
 *       Added under v12 WITH a layout change of mnerf_rays (tgt_height / tgt_width appended before the pad: the offsets of the older
 *       fields are unchanged, sizeof grows by 8) and one export, mnerf_box_downsample.  The version number stays 12; a binding built
 *       against the older layout is caught by mnerf_struct_size(1), which every binding is expected to compare before its first call.
 *       Added under v12 without a layout change: mnerf_debug_launch_plan (which kernel instance a problem size selects, host only);
 *       mnerf_debug_set_knob knows "wa_min4".
 *       Added under v12 without a layout change: caller-supplied rays (matchnerf_amd/csrc/free_rays.hip) - ray bundles of
 *       MNERF_RAY_FLOATS floats per ray, mnerf_cost_volume_rays, mnerf_ray_samples_rays, mnerf_render_rays_workspace_bytes,
 *       mnerf_render_rays, and the camera models that fill a bundle on the device: mnerf_camera - struct index
 *       MNERF_STRUCT_CAMERA -, mnerf_camera_rays.
 *       Added under v12 without a layout change: geometry export (matchnerf_amd/csrc/fusion.hip) - mnerf_depth_consistency,
 *       mnerf_point_cloud_workspace_bytes, mnerf_point_cloud, mnerf_depth_colormap.  No new struct: poses travel as mnerf_view.
 */
#ifndef MNERF_H_
#define MNERF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNERF_ABI_VERSION 12
#define MNERF_MAX_VIEWS 16
#define MNERF_FEAT_CH 128 /* channels of one pair-specific GMFlow feature map */
/* floats per sample of a `cond` buffer: sum(cos_n_group) + 4 n_views + 1, rounded up to a multiple of 8.
 * 16 views x ([8,8] groups) = 81 -> 88 fits the split weight-stream formats; the exact-f32 stream keeps its FiLM
 * inputs in registers and is limited to 64 (13 views with the shipped [2,8] groups). */
#define MNERF_COND_STRIDE_MAX 96
#define MNERF_COND_STRIDE_MAX_F32 64

enum {
  MNERF_OK = 0,
  MNERF_E_NULL = -1,        /* required pointer is NULL                         */
  MNERF_E_RANGE = -2,       /* a size / count is out of the supported range     */
  MNERF_E_UNSUPPORTED = -3, /* valid in the reference, not built in this kernel */
  MNERF_E_ALIGN = -4        /* pointer not aligned as required (16 B)           */
};

/* One source view (models/matchnerf.py:75-86 `ref_poses`). */
typedef struct mnerf_view {
  float extr[12]; /* world->camera [R|t], row-major 3x4  (batch.extrinsics[:, v, :3, :]) */
  float intr[9];  /* 3x3 intrinsics                       (batch.intrinsics[:, v])        */
  float near_, far_;
} mnerf_view;

/* The rays of one chunk of one target view.
 * Replaces camera.get_center_and_ray + sample_depth + get_3D_points_from_depth, which the
 * reference evaluates for the FULL image on every chunk (models/matchnerf.py:104-115,
 * misc/camera.py:255-286): here each ray is rebuilt in-kernel from the pixel index. */
typedef struct mnerf_rays {
  int32_t n_rays;         /* rays in this chunk                                               */
  int32_t n_samples;      /* S = opt.nerf.sample_intvs                                        */
  int32_t ray_begin;      /* first pixel index (row-major y*tgt_width+x) when ray_idx == NULL  */
  int32_t legacy_coord;   /* opt.nerf.legacy_coord: integer pixel centres, i/(S-1) depths      */
  int32_t depth_inverse;  /* opt.nerf.depth.param == "inverse"                                 */
  int32_t height, width;  /* image size of the SOURCE views (scene->images, the normalisation of projected coordinates) */
  const int32_t* ray_idx; /* device, [n_rays] pixel indices of the target grid (train / test-optim), or NULL */
  const float* strat_u;   /* device, [n_rays, S] U[0,1) offsets (stratified train), or NULL    */
  float kinv[9];          /* inverse target intrinsics, fp32 (camera.py:221-222)              */
  float c2w[12];          /* target camera->world 3x4 (legacy: fp64 inverse cast to fp32,      */
                          /* camera.py:231-240; else [R^T | -R^T t], camera.py:36-42)          */
  float near_, far_;      /* target near / far (batch.near_fars[:, -1])                       */
  /* POSE TABLE (ABI v7; video paths of small frames, models/matchnerf.py:42-71): several target poses in ONE launch.
   * With pose_table != NULL the launch's rays are the concatenation of the poses' frames: global ray g = ray_begin + r
   * renders pixel g % rays_per_pose of pose g / rays_per_pose, and kinv / c2w / near_ / far_ above are ignored in favour
   * of row `pose` of the table: [kinv 9 | c2w 12 | near | far | pad] = MNERF_POSE_FLOATS fp32.  rays_per_pose must be a
   * multiple of 64 (so that a wavefront never straddles two poses); ray_idx and strat_u must be NULL.  Accepted by
   * mnerf_cost_volume (<= 5 views), mnerf_decoder_chunk (split-fp16 stream, S <= 128, <= 5 views) and mnerf_render_chunk
   * (staged form) where mnerf_render_takes_pose_table() returns 1; MNERF_E_UNSUPPORTED everywhere else. */
  const float* pose_table;
  int32_t rays_per_pose;
  /* TARGET GRID: the pixel grid the rays are cast through, which need not be the source views' (a fly-through at another
   * resolution, a preview, a crop, a supersampled frame: kinv belongs to this grid).  Pixel indices - ray_begin, ray_idx, the
   * frames of a pose table (rays_per_pose = tgt_height * tgt_width is the caller's business) - decode with tgt_width; height /
   * width above keep describing the source images.  0, 0 = the views' size.  Both zero or both >= 1 (MNERF_E_RANGE otherwise);
   * with ray_idx == NULL and no pose table, ray_begin >= 0 and ray_begin + n_rays <= tgt_height * tgt_width.  Every entry point
   * works on a copy with the zeros replaced.  Forward entry points only: mnerf_cost_volume_backward answers
   * MNERF_E_UNSUPPORTED to a target grid that differs from the views' size. */
  int32_t tgt_height, tgt_width;
  int32_t pad_;
} mnerf_rays;
#define MNERF_POSE_FLOATS 24

/* Source-view data resident in HBM.  Feature maps are PAIR-MAJOR and CHANNEL-LAST:
 *   feat[s] : [n_pairs][2][fh[s]][fw[s]][128] fp32,  pair p=(a,b), a<b lexicographic,
 *             side 0 = feature of view a, side 1 = feature of view b after the GMFlow
 *             transformer ran on (a,b)  (models/gmflow/gmflow.py:47-67).
 * The reference keeps them as per-view channel chunks [V,(V-1)*128,h,w] (matchnerf.py:192-205)
 * and pairs chunk j of view i with chunk i of view j+1 (matchnerf.py:260-268) — the same data.
 *   images  : [n_views][H][W][4] fp32, RGB in [0,1] + one pad float (16-byte texels). */
typedef struct mnerf_scene {
  int32_t n_views;
  int32_t n_scales;       /* 2: raw 1/8 features + up-sampled 1/4 features                    */
  int32_t fh[2], fw[2];
  int32_t n_group[2];     /* opt.encoder.cos_n_group, each in {1,2,4,8}                        */
  const float* feat[2];
  const float* images;
  mnerf_view views[MNERF_MAX_VIEWS];
  /* ABI v9: operand image of feat[] for the MATRIX FORM of the cost volume (mnerf_cost_volume_operands below), or NULL.
   * With it, mnerf_cost_volume / mnerf_render_chunk interpolate the 128 channels of every (pair, scale) on the matrix pipe
   * (v_mfma_f32_32x32x16_f16, split-fp16 operands) for launches over contiguous pixels of one pose (ray_idx == NULL, no pose
   * table); every other launch, and a NULL pointer, takes the segment walk on feat[] - which must stay valid either way
   * (the backward kernels and the walk read it). */
  const void* feat_op;
} mnerf_scene;

/* Decoder parameters, pre-packed by the host (matchnerf_amd/cond_nerf.py):
 *   wstream : MFMA A-operand fragments of every Linear of CondNeRF in consumption order
 *             (layout in DESIGN.md §Decoder weight stream); 16-byte aligned.  Two formats:
 *             MNERF_WSTREAM_F32   fp32 fragments for v_mfma_f32_32x32x2_f32 (pack_wstream)
 *             MNERF_WSTREAM_BF16X3 each fp32 weight as three bf16 terms for
 *                                 v_mfma_f32_32x32x16_bf16, six product terms per MAC, fp32
 *                                 accumulate, fp32 bias fragments (pack_wstream16)
 *             MNERF_WSTREAM_F16X2 each fp32 weight as two fp16 terms of 2^ew W (one power-of-two
 *                                 scale per tensor) for v_mfma_f32_32x32x16_f16, three product terms
 *                                 per MAC, per-sample power-of-two activation gains chosen in the
 *                                 kernel, fp32 accumulate and biases (pack_wstream_h; default)
 *   small   : ray-transformer + density-head parameters (fp32, layout in DESIGN.md)
 * Architecture switches mirror opt.decoder.* / opt.nerf.* (configs/base.yaml:29-48). */
#define MNERF_WSTREAM_F32 0
#define MNERF_WSTREAM_BF16X3 1
#define MNERF_WSTREAM_F16X2 2
#define MNERF_WSTREAM_F16X1 3 /* ABI v8: the F16X2 stream read as plain fp16 weights (hi terms only), ONE product per MAC on fp16
                                * activations, fp32 accumulation: the reduced-precision FAST mode (RGB L-inf ~4e-3 against the
                                * fp32 path: outside the 1e-4 parity gate, never the default).  Ping-pong decoder only (<= 5
                                * source views, sample_intvs <= 128, no pose table); MNERF_E_UNSUPPORTED elsewhere. */

typedef struct mnerf_decoder {
  const float* wstream;
  int64_t wstream_floats;
  const float* small_;
  int32_t n_views;         /* V = opt.n_src_views                                               */
  int32_t cond_dim;        /* sum(cos_n_group) + 4*V (cond_nerf.py:18)                          */
  int32_t cond_stride;     /* floats per sample in `cond` buffers: multiple of 8, > cond_dim, <= MNERF_COND_STRIDE_MAX[_F32] */
  int32_t L_3D;            /* opt.decoder.posenc.L_3D (L_view must be 0)                        */
  int32_t raytrans_posenc; /* opt.decoder.raytrans_posenc                                       */
  int32_t raytrans_elu;    /* opt.decoder.raytrans_act == "ELU" (else ReLU)                     */
  int32_t density_maskfill;/* opt.decoder.density_maskfill                                      */
  int32_t wo_render_interval; /* opt.nerf.wo_render_interval                                    */
  int32_t setbg_opaque;    /* MatchNeRF.nerf_setbg_opaque                                       */
  int32_t wstream_format;  /* MNERF_WSTREAM_*                                                    */
} mnerf_decoder;

int mnerf_abi_version(void);
const char* mnerf_last_error(void);
/* sizeof() of the argument structs as compiled (0 view, 1 rays, 2 scene, 3 decoder, 4 encoder_layer, 5 conv, .. 10 lpips_weights: the
 * structs that prototypes name by type, in the order a binding mirrors them; MNERF_STRUCT_CAMERA mnerf_camera; -1 else):
 * lets a foreign-language binding verify its struct mirrors before the first call. */
int64_t mnerf_struct_size(int32_t which);

/* a8-a10 — target rays, depth samples, world points and their (u,v,z) in one source view.
 * Replaces camera.get_center_and_ray (misc/camera.py:255-278), MatchNeRF.sample_depth
 * (models/matchnerf.py:163-181), get_3D_points_from_depth (camera.py:281-286) and
 * get_coord_ref_ndc (camera.py:351-379).  Any of pts [R,S,3], ndc [R,S,3], depth [R,S] may be
 * NULL.  Bit-exact against the reference's CPU path (same k-ordered FMA chains). */
int mnerf_ray_samples(const mnerf_rays* rays, const mnerf_view* view, float* pts, float* ndc,
                      float* depth, void* stream);

/* K5 — volume-rendering quadrature.  Replaces NeRF.composite
 * (models/rfdecoder/nerf.py:101-124).  rgb_s [R,S,3], sigma [R,S], depth_s [R,S],
 * ray_len [R] (|ray|, only read when wo_render_interval == 0; may be NULL otherwise)
 * -> rgb [R,3], depth [R], opacity [R] and, when non-NULL, prob [R,S] (the per-sample weights
 * T_j alpha_j that the reference returns as its fourth value, nerf.py:116,124). */
int mnerf_composite(int32_t n_rays, int32_t n_samples, const float* rgb_s, const float* sigma,
                    const float* depth_s, const float* ray_len, int32_t wo_render_interval,
                    int32_t setbg_opaque, float* rgb, float* depth, float* opacity, float* prob,
                    void* stream);

/* K1+K2 — epipolar feature sampling + group-cosine cost volume + colours + visibility mask.
 * Replaces MatchNeRF.query_cond_info (models/matchnerf.py:209-293), sample_features_by_grid
 * (models/gmflow/utils.py:131-134) and get_coord_ref_ndc (misc/camera.py:351-379).
 * cond [n_rays*S, cond_stride]: [cos@scale0 | cos@scale1 | rgb_v0.. | mask_v0.. | 1.0 | 0 pad]
 * (the order CondNeRF concatenates them in, cond_nerf.py:59; the trailing 1.0 feeds the
 * bias column of the packed FiLM layer). */
int mnerf_cost_volume(const mnerf_scene* scene, const mnerf_rays* rays, int32_t cond_stride,
                      float* cond, void* stream);

/* ABI v9 — operand image for the matrix form of K1+K2: the feature maps of scene->feat[] re-laid for the matrix pipe, once per
 * source set (two launches, ~0.1 ms at 3 views of 512x640; enqueue-only).  Every fp32 texel x becomes two fp16 terms of 2^e x
 * (one power-of-two gain per map, taken from the map's largest magnitude, so that the cosine - which is scale-free per map -
 * is unchanged); texels are stored in aligned 2-row x 4-column cells, channel-tile-major, so that the 16 texels of a 4 x 4
 * chunk are the K dimension of one v_mfma_f32_32x32x16_f16 A operand per 32 channels, read with fully coalesced 16-byte loads
 * (layout: matchnerf_amd/csrc/cost_volume_mm.hip).  `opnd`: caller-owned, 16-byte aligned, mnerf_cost_volume_operand_bytes(scene)
 * bytes (about the size of the fp32 maps); scene->feat_op is ignored by both functions.  Replaces nothing in the reference: it
 * is the layout change that lets sample_features_by_grid (models/gmflow/utils.py:131-134) run as a matrix product. */
int64_t mnerf_cost_volume_operand_bytes(const mnerf_scene* scene);
int mnerf_cost_volume_operands(const mnerf_scene* scene, void* opnd, void* stream);

/* K3+K4+K5 — conditional radiance MLP, per-ray transformer and compositing for one chunk.
 * Replaces CondNeRF.forward (models/rfdecoder/cond_nerf.py:52-100), MultiHeadAttention
 * (ray_transformer.py:29-79), the ref-view-0 NDC warp and view-direction rotation
 * (models/matchnerf.py:118-132) and NeRF.composite (nerf.py:101-124).
 * view0 = source view 0 (coordinate reference).  cond as produced by mnerf_cost_volume.
 * Outputs rgb [R,3], depth [R], opacity [R]; dbg_rgb_s [R,S,3] / dbg_sigma [R,S] receive the
 * per-sample decoder outputs when non-NULL (parity tests). */
/* expected wstream size in 4-byte words for a format (negative: cannot be scheduled) */
int64_t mnerf_decoder_wstream_floats(int32_t cond_dim, int32_t cond_stride, int32_t L_3D,
                                     int32_t wstream_format);
int mnerf_decoder_chunk(const mnerf_decoder* dec, const mnerf_view* view0, const mnerf_rays* rays,
                        const float* cond, float* rgb, float* depth, float* opacity,
                        float* dbg_rgb_s, float* dbg_sigma, void* stream);

/* K3+K4 with caller-supplied inputs — the literal CondNeRF.forward(opt, points_3D, ray_unit, cond_info)
 * (models/rfdecoder/cond_nerf.py:52-100): x_ndc [R,S,3] sample coordinates w.r.t. source view 0
 * (matchnerf.py:121-126), dir [R,S,3] unit view directions in that view's frame (matchnerf.py:129-132),
 * cond [R*S, cond_stride] = cat(feat_info, color_info, mask_info) (+ the constant 1 and zero padding of
 * mnerf_cost_volume's layout) -> rgb_s [R,S,3], sigma [R,S].  Same kernel as mnerf_decoder_chunk without
 * the in-kernel ray geometry and without compositing; `legacy_coord` selects the positional-encoding
 * frequencies (2^l vs 2^l pi) and must match the packing of dec->wstream. */
int mnerf_decoder_samples(const mnerf_decoder* dec, int32_t n_rays, int32_t n_samples,
                          int32_t legacy_coord, const float* x_ndc, const float* dir,
                          const float* cond, float* rgb_s, float* sigma, void* stream);

/* a7 — one full render chunk = cost volume + decoder + compositing
 * (MatchNeRF.render, models/matchnerf.py:88-143).  Two forms with identical results, bit for bit:
 *   mnerf_render_chunk        staged: mnerf_cost_volume -> `workspace` -> mnerf_decoder_chunk (two launches);
 *                             `workspace` must hold mnerf_render_workspace_bytes(n_rays, n_samples, cond_stride)
 *                             bytes.  The default because it is the faster one on MI355X.
 *   mnerf_render_chunk_fused  ONE launch: the ray-chunk kernel produces the conditioning rows of each tile in LDS
 *                             and consumes them there (no HBM hand-off, no workspace).  Available where
 *                             mnerf_render_chunk_is_fused() returns 1: split-fp16 weight stream, S <= 128, at most
 *                             5 views / 32 conditioning inputs, cos_n_group entries >= 2; MNERF_E_UNSUPPORTED
 *                             otherwise.  MNERF_RENDER_FUSED=1 (read at load) makes mnerf_render_chunk take this
 *                             form wherever it is available (`workspace` may then be NULL). */
int64_t mnerf_render_workspace_bytes(int32_t n_rays, int32_t n_samples, int32_t cond_stride);
int32_t mnerf_render_chunk_is_fused(const mnerf_scene* scene, const mnerf_decoder* dec, const mnerf_rays* rays);
/* 1 if mnerf_render_chunk accepts a mnerf_rays.pose_table for this scene / decoder / sample count / frame size (rays_per_pose
 * = H*W): the kernel instances that take a table are the ones of the shipped shape (<= 5 source views, split-fp16 stream,
 * sample_intvs <= 128, H*W a multiple of 64).  A caller renders pose by pose otherwise. */
int32_t mnerf_render_takes_pose_table(const mnerf_scene* scene, const mnerf_decoder* dec, int32_t n_samples,
                                      int32_t rays_per_pose);
int mnerf_render_chunk(const mnerf_scene* scene, const mnerf_decoder* dec, const mnerf_rays* rays,
                       void* workspace, float* rgb, float* depth, float* opacity, void* stream);
int mnerf_render_chunk_fused(const mnerf_scene* scene, const mnerf_decoder* dec, const mnerf_rays* rays,
                             float* rgb, float* depth, float* opacity, void* stream);

/* Box filter of a supersampled frame: src [k*h, k*w, channels] fp32 row-major (what a render chunk sequence leaves for one frame:
 * channels = 3 for rgb, 1 for depth / opacity) -> dst [h, w, channels].  Each output value is the sum of its k x k block taken in
 * row-major order with sequential fp32 additions, multiplied by fp32(1 / (k*k)): a fixed order, so that a float32 restatement on
 * the host gives the same bits.  1 <= k <= 8, channels in {1, 3}, h, w >= 0 (MNERF_E_RANGE otherwise).  Enqueue-only, one thread
 * per output value.  Replaces nothing in the reference, which renders at the views' size only. */
int mnerf_box_downsample(const float* src, int32_t h, int32_t w, int32_t channels, int32_t k, float* dst, void* stream);

/* CALLER-SUPPLIED RAYS (added under v12).  Everything above rebuilds a target ray in-kernel from a pixel index of a pinhole camera
 * (kinv / c2w of mnerf_rays).  The entry points below take the rays themselves, as a RAY BUNDLE:
 *   ray_od : device, [n_rays][MNERF_RAY_FLOATS] fp32, 32-byte rows, 16-byte aligned (MNERF_E_ALIGN otherwise); a row is
 *            ox oy oz 0 | dx dy dz 0 = world origin and UN-NORMALISED world direction (the two pad floats are not read).
 * A sample is o + t d, with t from the launch's near_ / far_ / n_samples / legacy_coord / depth_inverse / strat_u exactly as for
 * pixel rays (MatchNeRF.sample_depth, models/matchnerf.py:163-181).  Compositing scales the intervals by |d| (nerf.py:101-124), so
 * pinhole rows - camera-z = 1 - reproduce the pixel paths' numbers, and unit directions make t, and the returned depth, a
 * Euclidean distance.
 * Of the mnerf_rays argument only n_rays, n_samples, legacy_coord, depth_inverse, height, width (the SOURCE views), near_, far_
 * and strat_u are read; ray_idx and pose_table must be NULL (MNERF_E_UNSUPPORTED); kinv, c2w, ray_begin and the target grid are
 * ignored (the functions work on a canonical copy: the pixel-range check of the target grid does not apply).  Enqueue-only; every
 * argument check precedes any HIP call (mnerf_render_rays: see there); n_rays == 0 is MNERF_OK and touches no buffer.  Forward only. */
#define MNERF_RAY_FLOATS 8
/* K1+K2 over a bundle: mnerf_cost_volume's rows (same layout, same bits for the same rays) by the 16-lane segment walk, whose
 * RayGeom is read from ray_od (two 16-byte loads per ray) instead of rebuilt from a pixel.  Always the walk: a scene whose
 * sum(cos_n_group) exceeds 16 is MNERF_E_UNSUPPORTED, scene->feat_op (the matrix form) is ignored.  Many views run in blocks of
 * view pairs as mnerf_cost_volume does. */
int mnerf_cost_volume_rays(const mnerf_scene* scene, const mnerf_rays* rays, const float* ray_od, int32_t cond_stride, float* cond,
                           void* stream);
/* The decoder's geometric inputs and the compositing's, per sample: x_ndc [R,S,3] sample coordinates w.r.t. source view 0
 * (matchnerf.py:121-126), dir [R,S,3] the ray's unit direction d / max(|d|, 1e-12) rotated into view0's frame (matchnerf.py:129-132),
 * depth_s [R,S] the sample parameters t, ray_len [R] = |d|.  Any output may be NULL; view0 is required for x_ndc and dir. */
int mnerf_ray_samples_rays(const mnerf_rays* rays, const float* ray_od, const mnerf_view* view0, float* x_ndc, float* dir,
                           float* depth_s, float* ray_len, void* stream);
/* One render chunk over a bundle = mnerf_cost_volume_rays -> mnerf_ray_samples_rays -> mnerf_decoder_samples -> mnerf_composite on
 * one stream (four launches, plus one per further pair block), through `workspace` (16-byte aligned,
 * mnerf_render_rays_workspace_bytes(n_rays, n_samples, dec->cond_stride) bytes; -1 for a negative / zero size).  Workspace layout,
 * every area starting 16-byte aligned (its float count rounded up to a multiple of 4), R = n_rays, S = n_samples:
 *   cond [R S cond_stride] | x_ndc [R S 3] | dir [R S 3] | depth_s [R S] | rgb_s [R S 3] | sigma [R S] | ray_len [R]
 * - the per-sample stages stay readable there after the call (parity tests).  Accepts the decoder shapes mnerf_decoder_samples
 * accepts; rgb [R,3], depth [R], opacity [R] as mnerf_render_chunk.  The matrix-form cost volume and the one-launch form have no
 * bundle instance.  Checked before the first launch: the structs, the bundle, the workspace, the outputs, the scene, and of the
 * decoder its weight pointers, the sample count and the weight stream's size for its shape and format; what only the decoder's own
 * dispatch can tell (a format without an instance for this shape) is answered by its step, after the first two were enqueued - as
 * in mnerf_render_chunk. */
int64_t mnerf_render_rays_workspace_bytes(int32_t n_rays, int32_t n_samples, int32_t cond_stride);
int mnerf_render_rays(const mnerf_scene* scene, const mnerf_decoder* dec, const mnerf_rays* rays, const float* ray_od,
                      void* workspace, float* rgb, float* depth, float* opacity, void* stream);

/* Camera models that fill a bundle on the device, one thread per pixel of a height x width grid (row-major pixel index
 * y * width + x; pixel centres (x, y) = integer coordinates with legacy_coord, + 0.5 otherwise, as for pixel rays):
 *   PINHOLE  origin = c2w's translation, direction = c2w [kinv (x,y,1); 1] - origin: the rows are, bit for bit, the rays the pixel
 *            entry points rebuild in-kernel (misc/camera.py:255-278)
 *   FISHEYE  equidistant: (xn, yn, .) = kinv (x,y,1), theta = |(xn, yn)| radians off the optical axis, camera direction
 *            (sin(theta) xn / theta, sin(theta) yn / theta, cos(theta)) ((0, 0, 1) at theta = 0), rotated by c2w: unit
 *   SPHERE   equirectangular window: lon = lon0 + u (lon1 - lon0) over the columns, lat = lat0 + v (lat1 - lat0) over the rows,
 *            (u, v) = (x / (width - 1), y / (height - 1)) with legacy_coord and (x / width, y / height) otherwise; lon_lat =
 *            {lon0, lon1, lat0, lat1} in radians, a full panorama is -pi, pi, -pi/2, pi/2; camera direction (cos(lat) sin(lon),
 *            sin(lat), cos(lat) cos(lon)) - x right, y down, z forward -, rotated by c2w: unit.  kinv is not read
 *   ORTHO    origin = c2w (xn, yn, 0, 1), direction = c2w's z axis normalised: parallel rays, kinv scales pixels to world units
 * Sines and cosines are the library's own (angles reduced in revolutions with a two-float 1 / (2 pi), abs error 3e-7), the
 * camera -> world products the k-ordered FMA chains of the projection code.  lon_lat is read by SPHERE only. */
#define MNERF_CAM_PINHOLE 0
#define MNERF_CAM_FISHEYE 1
#define MNERF_CAM_SPHERE 2
#define MNERF_CAM_ORTHO 3
typedef struct mnerf_camera {
  int32_t model, height, width, legacy_coord;
  float kinv[9];
  float c2w[12];
  float lon_lat[4];
} mnerf_camera;
#define MNERF_STRUCT_CAMERA 32 /* mnerf_struct_size(MNERF_STRUCT_CAMERA) = sizeof(mnerf_camera) */
/* rows [0, n_pixels) of ray_od <- pixels [pixel_begin, pixel_begin + n_pixels) of the camera's grid (MNERF_E_RANGE outside it).
 * `camera` points at a mnerf_camera (host memory, read during the call).  It travels as an untyped pointer: the structs that
 * prototypes name by type stay the eleven of mnerf_struct_size(0..10), which existing bindings mirror and count; a binding checks
 * its mirror of this one against mnerf_struct_size(MNERF_STRUCT_CAMERA). */
int mnerf_camera_rays(const void* camera, int32_t pixel_begin, int32_t n_pixels, float* ray_od, void* stream);

/* Backward kernels of the ray chunk (training through the HIP path; reference: autograd through the eager chain,
 * coach.py:215-243).
 * K5 backward — given d(rgb [R,3], depth [R] or NULL, opacity [R] or NULL) and the forward's per-sample inputs,
 * writes g_rgb_s [R,S,3] and g_sigma [R,S] (NeRF.composite, nerf.py:101-124). */
int mnerf_composite_backward(int32_t n_rays, int32_t n_samples, const float* rgb_s, const float* sigma,
                             const float* depth_s, const float* ray_len, int32_t wo_render_interval,
                             int32_t setbg_opaque, const float* g_rgb, const float* g_depth,
                             const float* g_opacity, float* g_rgb_s, float* g_sigma, void* stream);
/* K1+K2 backward — g_cond [n_rays*S, cond_stride] (gradient of mnerf_cost_volume's rows; only the cosine
 * entries are read) is scattered into the feature-map gradients g_feat0 / g_feat1 (layouts of scene->feat[0] /
 * feat[1]; ACCUMULATED with atomic adds: the caller zero-fills them; g_feat1 may be NULL when n_scales == 1).
 * The forward interpolation is recomputed from `scene` and `rays` (query_cond_info, matchnerf.py:209-293).  Training renders at
 * the views' size: a rays->tgt_height / tgt_width that differs from it is MNERF_E_UNSUPPORTED. */
int mnerf_cost_volume_backward(const mnerf_scene* scene, const mnerf_rays* rays, int32_t cond_stride,
                               const float* g_cond, float* g_feat0, float* g_feat1, void* stream);

/* Test / diagnosis hook: set one tuning knob after load (the lower-case name of its MNERF_* environment variable without the
 * prefix: "decoder_pp", "cv_variant", ...).  Returns MNERF_OK and the previous value through *old_value (may be NULL), or
 * MNERF_E_RANGE + a message for an unknown name (ABI v6: the status no longer shares the return value with the old value,
 * whose legitimate range includes -1).  The table is the library's only mutable process-wide state besides the thread-local
 * error string; this hook is its only writer.  Writes and the launches' reads are serialised by a lock and every launch works
 * on a copy of the table, so a launch on another thread sees the value from before or after the call, never a torn table;
 * kernels already enqueued are not affected. */
int mnerf_debug_set_knob(const char* name, int value, int* old_value);

/* Test / diagnosis hook: the kernel instance that a launch of the given problem would select, from the very function the launch
 * calls.  Host only: no device is touched and nothing is launched, so it answers on a machine without a GPU.  `what` names the
 * dispatcher, `args` its n_args problem sizes, `plan` receives the selection (n_plan >= the number of values listed):
 *   "conv2d"            c_in, c_out, ksize, stride, n_img, h_in, w_in, in_channels_last, upsample2x
 *                       -> NMB, TPW, CL of conv_kernel<NMB, TPW, CL>, and the number of 128-channel blocks (grid.y)
 *   "conv_gemm"         fwd (1: mnerf_conv2d_forward_f32, 0: mnerf_conv2d_backward_data), n_img, c_in, c_out, h_in, w_in, ksize, stride
 *                       -> CIB, NB, TAIL, FWD of conv_gemm_kernel (TAIL: a source channel count that is no multiple of 8)
 *   "conv_wgrad"        n_img, c_in, c_out, h_in, w_in, ksize, stride
 *                       -> chunks, rows of dY per chunk (mnerf_conv2d_backward_weight and ..._f16x3 alike)
 *   "instance_norm", "instance_norm_backward"   plane_size, aligned (1: all buffers 16-byte aligned)
 *                       -> THREADS, VPT of the register-cached instance, or 0, 0 for the streaming kernel
 *   "window_attention"  batch, h, w, num_splits
 *                       -> 4 or 2: query waves per workgroup (every arithmetic of mnerf_window_attention and the pre-split /
 *                          images forms take the same rule; it reads the knob "wa_min4")
 * Returns MNERF_OK, MNERF_E_RANGE for an unknown name, a wrong count or a size out of range, MNERF_E_UNSUPPORTED for channel
 * counts, filters or strides that the convolution entry points do not build.  The query answers the selection only: it does not
 * repeat every argument check of the launch (buffers, alignment, workspace, layouts), so MNERF_OK is no promise that a launch of
 * that problem is accepted. */
int mnerf_debug_launch_plan(const char* what, const int64_t* args, int32_t n_args, int32_t* plan, int32_t n_plan);

/* K3+K4 backward — gradients of the conditional MLP + ray transformer (CondNeRF.forward, cond_nerf.py:52-100;
 * MultiHeadAttention.forward, ray_transformer.py:29-79; what `loss.backward()` does to them in coach.py:215-243).
 * The parameters are given in torch's own layouts (Linear.weight [out,in], fp32), indexed by MNERF_DT_*; `g[k]` receives the
 * gradient of `w[k]`, ACCUMULATED (the caller zero-fills or carries over), NULL = not wanted. */
enum {
  MNERF_DT_PTS_W0 = 0,   /* pts_linears.i.weight = 2 i, .bias = 2 i + 1, i = 0..5 */
  MNERF_DT_BIAS_W = 12,  /* pts_bias (the FiLM multiplier) */
  MNERF_DT_BIAS_B,
  MNERF_DT_ALPHA_W,      /* alpha_linear.0 */
  MNERF_DT_ALPHA_B,
  MNERF_DT_WQ,           /* ray_attention.w_qs / w_ks / w_vs / fc (.weight, no bias) */
  MNERF_DT_WK,
  MNERF_DT_WV,
  MNERF_DT_FC,
  MNERF_DT_LN_W,         /* ray_attention.layer_norm */
  MNERF_DT_LN_B,
  MNERF_DT_OA0_W,        /* out_alpha_linear.0 */
  MNERF_DT_OA0_B,
  MNERF_DT_OA2_W,        /* out_alpha_linear.2 */
  MNERF_DT_OA2_B,
  MNERF_DT_FEAT_W,       /* feature_linear */
  MNERF_DT_FEAT_B,
  MNERF_DT_VIEWS_W,      /* views_linears.0 : [64, 128 + 3] */
  MNERF_DT_VIEWS_B,
  MNERF_DT_RGB_W,        /* rgb_linear */
  MNERF_DT_RGB_B,
  MNERF_DEC_TENSORS
};
typedef struct mnerf_decoder_train {
  int32_t n_views;          /* source views: the last n_views of the cond_dim conditioning columns are the visibility masks */
  int32_t cond_dim;         /* conditioning columns the FiLM Linear reads */
  int32_t n_trunk;          /* opt.decoder.net_depth (6) */
  int32_t net_width;        /* opt.decoder.net_width (128) */
  int32_t skip_layer;       /* the trunk layer after which the encoding is concatenated again (opt.decoder.skip[0]); -1: none */
  int32_t L_3D;             /* octaves of the positional encoding */
  int32_t legacy_coord;     /* opt.nerf.legacy_coord: frequency 2^l and [l][xyz] order instead of pi 2^l and [xyz][sin|cos][l] */
  int32_t raytrans_elu;     /* opt.decoder.raytrans_act == 'ELU' (else ReLU) */
  int32_t raytrans_posenc;  /* add raytrans_table [S,16] to the alpha features */
  int32_t density_maskfill;
  const float* raytrans_table;
  const float* w[MNERF_DEC_TENSORS];
  float* g[MNERF_DEC_TENSORS];
} mnerf_decoder_train;
/* x_ndc [N,3] sample coordinates and dirs [n_rays,3] unit view directions in source view 0's frame (what mnerf_ray_samples and the
 * host compute for the forward), cond [N, cond_stride] the rows mnerf_cost_volume wrote, g_rgb_s [N,3] / g_sigma [N] from
 * mnerf_composite_backward (N = n_rays * n_samples, n_samples <= 256).  g_cond [N, cond_stride] (or NULL) receives the gradient
 * of the first cond_dim columns of the rows (other columns untouched).  workspace: mnerf_decoder_backward_workspace_bytes(). */
int64_t mnerf_decoder_backward_workspace_bytes(int32_t n_rays, int32_t n_samples);
int mnerf_decoder_backward(const mnerf_decoder_train* dec, int32_t n_rays, int32_t n_samples, const float* x_ndc,
                           const float* dirs, const float* cond, int32_t cond_stride, const float* g_rgb_s,
                           const float* g_sigma, float* g_cond, void* workspace, void* stream);

/* K6 — GMFlow single-head (shifted-)window attention, flash style (no score matrix).
 * Replaces single_head_split_window_attention / single_head_full_attention and the
 * shift-mask tensor (models/gmflow/transformer.py:8-16, 19-43, 46-105).
 * q,k,v,out [batch, h*w, 128]; num_splits >= 1 (1 = full attention); `shifted` applies the
 * swin roll by half a window with wrap-region masking (-100 added across regions).
 * `math`: MNERF_WA_SPLIT_BF16 (fp32-grade products from three bf16 terms per operand, six products per MAC on the
 * bf16 matrix cores), MNERF_WA_SPLIT_F16 (two range-managed fp16 terms,
 * three products; gains per query and per 32-key K / V tile) or MNERF_WA_EXACT_F32 (v_mfma_f32_32x32x2_f32). */
#define MNERF_WA_SPLIT_BF16 0
#define MNERF_WA_EXACT_F32 1
#define MNERF_WA_SPLIT_F16 2
int mnerf_window_attention(const float* q, const float* k, const float* v, float* out,
                           int32_t batch, int32_t h, int32_t w, int32_t num_splits,
                           int32_t shifted, int32_t math, void* stream);

/* K6 with the K / V matrix operands prepared once per call (the host's default): a first small kernel turns every
 * 32-key tile of every window into split-fp16 operand fragments + one power-of-two gain per tile and matrix in
 * `workspace`, the attention kernel streams those images through LDS (arithmetic = MNERF_WA_SPLIT_F16; its waves
 * no longer convert the window's K and V once per 32 queries).  Same arguments and semantics as above;
 * `workspace`: device, 16-byte aligned, at least mnerf_window_attention_workspace_bytes(batch, h, w, num_splits)
 * bytes (= the size of k and v together + 32 bytes per tile), scratch only - nothing is kept between calls. */
size_t mnerf_window_attention_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t num_splits);
int mnerf_window_attention_presplit(const float* q, const float* k, const float* v, float* out,
                                    int32_t batch, int32_t h, int32_t w, int32_t num_splits, int32_t shifted,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* q | k | v projections of a GMFlow transformer layer in one launch (models/gmflow/transformer.py:147-151):
 *   q = Wq x_q,  k = Wk x_kv',  v = Wv x_kv'      x_q, x_kv, q, k, v: [n_seq, seq_len, 128] fp32 tokens
 * kv_swap: x_kv' is x_kv with its two batch halves exchanged (sequence b reads sequence (b + n_seq/2) mod n_seq): the
 * "target" of the batched pair members (transformer.py:317-335) without building the concatenated tensor.
 * wstream: split-fp16 A-operand fragments of [Wq | Wk | Wv] (matchnerf_amd/gmflow.py: pack_qkv;
 * mnerf_qkv_wstream_floats() words, device), ew: the three weight-scale exponents (HOST array of 3). */
int64_t mnerf_qkv_wstream_floats(void);
int mnerf_qkv_projection(const float* wstream, const int32_t* ew, const float* x_q, const float* x_kv, int32_t kv_swap,
                         float* q, float* k, float* v, int32_t n_seq, int32_t seq_len, void* stream);

/* The same projections with K and V written directly as the window attention's operand images (no k / v tensors, no
 * operand pre-pass): q [batch, h*w, 128] fp32 + `workspace` in the format mnerf_window_attention_images consumes
 * (mnerf_window_attention_workspace_bytes(batch, h, w, num_splits) bytes).  The geometry arguments must be the ones the
 * attention call will get. */
int mnerf_qkv_window_images(const float* wstream, const int32_t* ew, const float* x_q, const float* x_kv, int32_t kv_swap,
                            float* q, void* workspace, size_t workspace_bytes, int32_t batch, int32_t h, int32_t w,
                            int32_t num_splits, int32_t shifted, void* stream);
/* K6 on a workspace filled by mnerf_qkv_window_images (or by a previous mnerf_window_attention_presplit call) */
int mnerf_window_attention_images(const float* q, float* out, int32_t batch, int32_t h, int32_t w, int32_t num_splits,
                                  int32_t shifted, const void* workspace, size_t workspace_bytes, void* stream);

/* K6 backward — gradients of the (shifted-)window attention (what `loss.backward()` does to
 * models/gmflow/transformer.py:46-105 in coach.py:215-243), flash style: the [windows, L_w, L_w] score tensor is never
 * materialised.  q, k, v, out (the forward's result), g_out (gradient of `out`): [batch, h*w, 128] fp32; g_q, g_k, g_v
 * (same shape) are OVERWRITTEN.  fp32-grade matrix products (MNERF_WA_BWD_MATH = "f16x3", the default: two fp16 terms per operand with
 * power-of-two gains from the tensors' maxima, three term products; "bf16x6": three bf16 terms, six term products; "f32": the
 * exact-f32 matrix instruction), deterministic (the only atomics are the maxima of the f16x3 form's gains).  `out` must be the
 * forward's result for these q, k, v (the f16x3 gains bound <g_out, out> by the maxima of g_out and v).  `workspace`: at least
 * mnerf_window_attention_backward_workspace_bytes(batch, h, w) bytes (four floats per token: row maximum, row sum of
 * exponentials, <g_out, out>, |g_out|^2; + the four operand maxima). */
int64_t mnerf_window_attention_backward_workspace_bytes(int32_t batch, int32_t h, int32_t w);
int mnerf_window_attention_backward(const float* q, const float* k, const float* v, const float* out, const float* g_out,
                                    float* g_q, float* g_k, float* g_v, int32_t batch, int32_t h, int32_t w,
                                    int32_t num_splits, int32_t shifted, void* workspace, size_t workspace_bytes,
                                    void* stream);
/* Training pair: the forward that also publishes the softmax's row statistics, row_stats = [2][batch * h*w] fp32 (running
 * maximum | sum of exponentials, log2 domain, token order), and the backward that reads them instead of recomputing them in a
 * first pass over all keys.  Same results as the pair above up to the last bits of the statistics. */
int mnerf_window_attention_presplit_stats(const float* q, const float* k, const float* v, float* out, float* row_stats,
                                          int32_t batch, int32_t h, int32_t w, int32_t num_splits, int32_t shifted,
                                          void* workspace, size_t workspace_bytes, void* stream);
int mnerf_window_attention_backward_stats(const float* q, const float* k, const float* v, const float* out, const float* g_out,
                                          const float* row_stats, float* g_q, float* g_k, float* g_v, int32_t batch, int32_t h,
                                          int32_t w, int32_t num_splits, int32_t shifted, void* workspace,
                                          size_t workspace_bytes, void* stream);

/* InstanceNorm2d (no affine, biased variance, as torch.nn.functional.instance_norm) of an NCHW tensor fused with what
 * follows it in the GMFlow backbone (models/gmflow/backbone.py:27-35, 101-103):
 *   v = (x - mean_plane) / sqrt(var_plane + eps);  if relu_inner: v = max(v, 0);
 *   if residual: v += residual;                     if relu_outer: v = max(v, 0)
 * x, residual (or NULL), out: [planes = N*C][plane_size = H*W] fp32; out may alias x.  One workgroup per plane.
 * out_absmax: absmax region (MNERF_ABSMAX_FLOATS floats, see mnerf_conv2d) or NULL; max |out| is merged into it (the
 * operand scale of the convolution that reads `out`). */
int mnerf_instance_norm(const float* x, const float* residual, float* out, int64_t planes, int64_t plane_size,
                        float eps, int32_t relu_inner, int32_t relu_outer, float* out_absmax, void* stream);

/* Backward of out = [relu](InstanceNorm(x)) (training path; what autograd runs for F.instance_norm + F.relu in
 * models/gmflow/backbone.py:27-35, 101-103): dx from x (the norm's INPUT, the statistics are re-derived) and dy.  relu: the forward
 * applied a ReLU to the normalised value.  x, dy, dx: [planes][plane_size] fp32; dx may alias dy. */
int mnerf_instance_norm_backward(const float* x, const float* dy, float* dx, int64_t planes, int64_t plane_size, float eps,
                                 int32_t relu, void* stream);

/* F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False) of the up-sampler's training path (superres.py:37) and its
 * backward.  in [planes][h][w] -> out [planes][2h][2w] (+ add, same shape as out, or NULL); dout [planes][2h][2w] -> din. */
int mnerf_upsample_bilinear2x(const float* in, const float* add, float* out, int64_t planes, int32_t h, int32_t w, void* stream);
int mnerf_upsample_bilinear2x_backward(const float* dout, float* din, int64_t planes, int32_t h, int32_t w, void* stream);

/* Convolutions of the GMFlow backbone / up-sampler (models/gmflow/backbone.py:6-122, superres.py:5-38) as implicit
 * GEMMs with fp32-grade split-fp16 products (matchnerf_amd/csrc/conv.hip).  Built: c_in a multiple of 32, c_out 64 /
 * 96 / 128, 1x1 and 3x3 filters with padding ksize/2, stride 1 / 2; and, for the VGG-16 of LPIPS (below), c_out 256 / 512 with
 * NCHW input and output and no added tensor: the output channels are split into blocks of 128 along a grid dimension, and wstream
 * is the concatenation of the blocks' streams, every block packed with the SAME ew (matchnerf_amd/gmflow.py: pack_conv_blocks).
 * This is the entry point through which the wide convolution is tested alone.
 *   wstream     : A-operand fragments of 2^ew * W, K16-step s = (tap, 16 input channels), unit (s, 32-row block) =
 *                 [hi | lo] x 64 lanes x 8 fp16 (matchnerf_amd/gmflow.py: pack_conv); mnerf_conv_wstream_floats() words
 *   bias        : [c_out] or NULL;  leaky_slope: LeakyReLU slope applied to the result (1 = none)
 * mnerf_conv2d: in [n_img, c_in, h_in, w_in] (or [n_img, h_in, w_in, c_in] with in_channels_last), optionally read
 * through a nearest 2x up-sampling (upsample2x); out [n_img, c_out, h_out, w_out] NCHW.
 *   in_absmax   : absmax region (MNERF_ABSMAX_FLOATS floats) whose maximum is >= max |in| (operands are scaled by ONE
 *                 power of two taken from it; a value that is too small overflows fp16) - filled by the producer of
 *                 `in`: mnerf_instance_norm, mnerf_conv2d (out_absmax) or mnerf_absmax
 *   add_bilinear2x : NULL, or [n_img, c_out, h_out/2, w_out/2] NCHW whose bilinear 2x up-sampling (align_corners=False,
 *                 as F.interpolate) is added to the result (superres.py:37: right = up(right) + conv(left))
 *   out_layout  : MNERF_CONV_OUT_NCHW, _CHANNEL_LAST (the transformer's tokens) or _PAIR_MAJOR (image i of the batched
 *                 pair members [a-sides; b-sides] goes to (pair i mod n_img/2, side i div n_img/2))
 *   add_channel_last : NULL, or a [h_out*w_out][c_out] tile added to every image of a channel-last result (the window
 *                 position embedding, gmflow/utils.py:68-88, fused into the backbone's last convolution)
 *   out_absmax  : absmax region or NULL; max |out| is merged into it with atomic maxima (zero it first). */
#define MNERF_ABSMAX_SLOTS 64   /* an "absmax region" = SLOTS partial maxima, STRIDE floats apart: 2048 floats, zeroed */
#define MNERF_ABSMAX_STRIDE 32  /* by the caller; producers merge with atomic maxima, the convolution reduces the slots */
#define MNERF_ABSMAX_FLOATS (MNERF_ABSMAX_SLOTS * MNERF_ABSMAX_STRIDE)
typedef struct mnerf_conv {
  const float* wstream;
  int64_t wstream_floats;
  const float* bias;
  int32_t c_in, c_out, ksize, stride;
  int32_t ew;
  float leaky_slope;
} mnerf_conv;
int64_t mnerf_conv_wstream_floats(int32_t c_in, int32_t c_out, int32_t ksize);
#define MNERF_CONV_OUT_NCHW 0
#define MNERF_CONV_OUT_CHANNEL_LAST 1 /* tokens [n_img][h_out][w_out][c_out] */
#define MNERF_CONV_OUT_PAIR_MAJOR 2   /* the cost volume's feature layout [n_img/2][2][h_out][w_out][c_out] */
int mnerf_conv2d(const mnerf_conv* cv, const float* in, int32_t in_channels_last, int32_t upsample2x,
                 const float* in_absmax, const float* add_bilinear2x, const float* add_channel_last, float* out,
                 int32_t out_layout, float* out_absmax, int32_t n_img, int32_t h_in, int32_t w_in, void* stream);
/* The backbone's stem: Conv2d(3, 64, 7, stride 2, padding 3, bias=False) (models/gmflow/backbone.py:45, 101), same
 * arithmetic as mnerf_conv2d.  wstream: fragments of the [64, 147 -> 160] matrix (k = 3 (7 ky + kx) + c;
 * matchnerf_amd/gmflow.py: pack_conv_stem; mnerf_conv_stem_wstream_floats() words).  in [n_img,3,h_in,w_in] ->
 * out [n_img,64,(h_in-1)/2+1,(w_in-1)/2+1] NCHW. */
int64_t mnerf_conv_stem_wstream_floats(void);
int mnerf_conv_stem(const float* wstream, int32_t ew, const float* in, const float* in_absmax, float* out,
                    int32_t n_img, int32_t h_in, int32_t w_in, void* stream);
/* max |x| of n floats merged into the absmax region `out` (atomic maxima; zero it first) */
int mnerf_absmax(const float* x, int64_t n, float* out, void* stream);

/* Backward of Conv2d(c_in, c_out, ksize, stride, padding = ksize / 2) for the training path of the GMFlow backbone / up-sampler
 * (what autograd runs for models/gmflow/backbone.py:6-122, superres.py:5-38 under coach.py:215-243); exact-fp32 products on
 * v_mfma_f32_32x32x2_f32, NCHW fp32 (matchnerf_amd/csrc/conv_backward.hip).  Built: c_in, c_out in {32, 64, 96, 128}, ksize 1 / 3,
 * stride 1 / 2.  h_in, w_in: the convolution's INPUT size; dy is [n_img, c_out, h_out, w_out] with h_out = (h_in + 2 (ksize/2) -
 * ksize) / stride + 1.
 *   mnerf_conv2d_backward_data  : dx [n_img, c_in, h_in, w_in] = conv_transpose(dy, W).  w_tap_major: the weight permuted to
 *                                 [ky][kx][c_out][c_in] (torch: weight.permute(2, 3, 0, 1).contiguous()).  dx is overwritten.
 *   mnerf_conv2d_backward_weight: dw [c_out, c_in, ksize, ksize] (torch's layout, overwritten) = sum over images and positions;
 *                                 partial sums of row chunks go through `workspace` (mnerf_conv2d_backward_weight_workspace_bytes)
 *                                 and are added in chunk order: bit-reproducible. */
int mnerf_conv2d_backward_data(const float* dy, const float* w_tap_major, float* dx, int32_t n_img, int32_t c_in, int32_t c_out,
                               int32_t h_in, int32_t w_in, int32_t ksize, int32_t stride, void* stream);
size_t mnerf_conv2d_backward_weight_workspace_bytes(int32_t n_img, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                                    int32_t ksize, int32_t stride);
int mnerf_conv2d_backward_weight(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes, int32_t n_img,
                                 int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, int32_t ksize, int32_t stride, void* stream);
/* The weight gradient on the 16-bit matrix pipe: operands as two fp16 terms with one power-of-two gain per tensor, three products per
 * MAC, fp32 accumulation (the forward kernels' arithmetic).  x_absmax / dy_absmax: absmax regions (MNERF_ABSMAX_FLOATS floats, see
 * mnerf_conv2d) holding max |x| and max |dy| - filled by mnerf_absmax or the tensors' producers.  Same workspace. */
int mnerf_conv2d_backward_weight_f16x3(const float* x, const float* dy, const float* x_absmax, const float* dy_absmax, float* dw,
                                       void* workspace, size_t workspace_bytes, int32_t n_img, int32_t c_in, int32_t c_out, int32_t h_in,
                                       int32_t w_in, int32_t ksize, int32_t stride, void* stream);
/* The training FORWARD of the same convolutions in exact fp32 (the gradients' arithmetic; no weight stream to re-pack after every
 * optimizer step): y [n_img, c_out, h_out, w_out] = conv(x, W) + bias.  w_tap_major: the weight permuted to [ky][kx][c_in][c_out]
 * (torch: weight.permute(2, 3, 1, 0).contiguous()); bias [c_out] or NULL.  c_in: any count up to 128 (the stem: 3), c_out a
 * multiple of 32 up to 128, ksize 1 / 3 / 7, stride 1 / 2. */
int mnerf_conv2d_forward_f32(const float* x, const float* w_tap_major, const float* bias, float* y, int32_t n_img, int32_t c_in,
                             int32_t c_out, int32_t h_in, int32_t w_in, int32_t ksize, int32_t stride, void* stream);
/* Weight gradient of the stem Conv2d(3, 64, 7, stride 2, padding 3) (backbone.py:45): dw [64, 3, 7, 7]; x [n_img, 3, h_in, w_in],
 * dy [n_img, 64, (h_in - 1) / 2 + 1, (w_in - 1) / 2 + 1].  (Its data gradient is the gradient of the images: never needed.) */
size_t mnerf_conv_stem_backward_weight_workspace_bytes(int32_t n_img, int32_t h_in, int32_t w_in);
int mnerf_conv_stem_backward_weight(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes, int32_t n_img,
                                    int32_t h_in, int32_t w_in, void* stream);

/* K7 — what follows the window attention inside one GMFlow transformer layer, as one kernel
 * (TransformerLayer.forward, models/gmflow/transformer.py:176-185):
 *   message = norm1(merge(attn));  [ffn:] message = norm2(mlp.2(GELU(mlp.0(cat[source, message]))));  out = source + message
 * attn, source, out: [n_tokens, 128] fp32 (out may alias neither input).  The three bias-free Linears travel as one
 * split-fp16 MFMA A-fragment stream (matchnerf_amd/gmflow.py: pack_encoder_block; layout in DESIGN.md section 5):
 * 32 KiB segments = 4 K16-steps x 4 row blocks x [hi | lo]; merge (2 segments), then per 128-unit hidden chunk
 * mlp.0 (4 segments: source features, then the message in accumulator order) and mlp.2 (2 segments).
 * ew_*: exponent of the power-of-two scale each weight tensor was packed with; ln: [4][128] = norm1 weight | norm1
 * bias | norm2 weight | norm2 bias (norm2 ignored when ffn == 0).  fp32-grade results (same arithmetic as the
 * decoder's MNERF_WSTREAM_F16X2 path). */
typedef struct mnerf_encoder_layer {
  const float* wstream;
  int64_t wstream_floats;  /* mnerf_encoder_block_wstream_floats(ffn) */
  const float* ln;
  int32_t ffn;             /* 0: self-attention layer (no FFN), 1: cross-attention + FFN layer */
  int32_t ew_merge, ew_w1, ew_w2;
} mnerf_encoder_layer;
int64_t mnerf_encoder_block_wstream_floats(int32_t ffn);
int mnerf_encoder_block(const mnerf_encoder_layer* blk, const float* attn, const float* source, float* out,
                        int32_t n_tokens, void* stream);

/* Backward of a transformer layer around the window attention (what `loss.backward()` does to
 * models/gmflow/transformer.py:108-185 in coach.py:215-243; round 4).  Parameters in torch's layouts, gradients ACCUMULATED
 * into the g_* tensors (a NULL g_* skips that parameter).  Matrix products with I, J >= 128 run fp32-grade in split-bf16 (three bf16 terms per operand,
 * six products per MAC on the bf16 MFMA) by default, exact f32 (v_mfma_f32_32x32x2_f32) with MNERF_GEMM_MATH=f32 or for smaller products
 * (csrc/gemm.hip). */
typedef struct mnerf_encoder_layer_train {
  int32_t ffn;            /* 0: self-attention layer (merge + norm1 only), 1: + cat / mlp / norm2 */
  int32_t pad_;
  const float* w_merge;   /* merge.weight [128,128] */
  const float* ln1_w;     /* norm1.weight / bias [128] */
  const float* ln1_b;
  const float* w_mlp0;    /* mlp.0.weight [1024,256] (columns: source | message) */
  const float* w_mlp2;    /* mlp.2.weight [128,1024] */
  const float* ln2_w;
  const float* ln2_b;
  float* g_w_merge;
  float* g_ln1_w;
  float* g_ln1_b;
  float* g_w_mlp0;
  float* g_w_mlp2;
  float* g_ln2_w;
  float* g_ln2_b;
} mnerf_encoder_layer_train;
/* attn (the attention's output), source (the layer's input), g_out (gradient of the layer's output): [n_tokens,128] ->
 * g_attn, g_source [n_tokens,128] (OVERWRITTEN; g_source includes the residual path).  The chain of mnerf_encoder_block is
 * re-evaluated in fp32 with its pre-activations kept in `workspace` (mnerf_encoder_layer_backward_workspace_bytes:
 * 3 970 floats per token). */
int64_t mnerf_encoder_layer_backward_workspace_bytes(int32_t n_tokens);
int mnerf_encoder_layer_backward(const mnerf_encoder_layer_train* layer, const float* attn, const float* source,
                                 const float* g_out, float* g_attn, float* g_source, int32_t n_tokens, void* workspace,
                                 void* stream);
/* Training pair (round 6): the forward that also writes the pre-norm activations - merge's output before norm1 (m1 [n_tokens,128])
 * and, for a layer with an FFN, mlp.0's output before the GELU (z1 [n_tokens,1024]) and mlp.2's output before norm2 (m2
 * [n_tokens,128]; NULL without an FFN); `out` equal to mnerf_encoder_block's bit for bit -, and the backward that reads them instead
 * of re-evaluating them (four of an FFN layer's eleven matrix products).  Same workspace. */
int mnerf_encoder_block_save(const mnerf_encoder_layer* blk, const float* attn, const float* source, float* out, float* m1,
                             float* z1, float* m2, int32_t n_tokens, void* stream);
int mnerf_encoder_layer_backward_saved(const mnerf_encoder_layer_train* layer, const float* attn, const float* source,
                                       const float* g_out, const float* m1, const float* z1, const float* m2, float* g_attn,
                                       float* g_source, int32_t n_tokens, void* workspace, void* stream);
/* q = x_q Wq^T, k = x_kv Wk^T, v = x_kv Wv^T (mnerf_qkv_projection without the batch swap: the caller passes the key / value
 * source it used):  g_xq = g_q Wq and g_xkv = g_k Wk + g_v Wv are OVERWRITTEN ([n_tokens,128], two different buffers),
 * gw_* [128,128] += g_*^T x_* (NULL: skipped). */
int mnerf_qkv_backward(const float* w_q, const float* w_k, const float* w_v, const float* x_q, const float* x_kv,
                       const float* g_q, const float* g_k, const float* g_v, float* g_xq, float* g_xkv, float* gw_q,
                       float* gw_k, float* gw_v, int32_t n_tokens, void* stream);

/* Test hook — the strided GEMM under the backward entry points above:  C[I,J] (mode 0: =, 1: +=, 2: atomic +=)
 * sum_k A(i,k) B(k,j) (+ bias[j]),  A(i,k) = a[i sa_i + k sa_k],  B(k,j) = b[k sb_k + j sb_j],  C row stride sc_i.
 * math 1 = split-bf16 on the 16-bit matrix instruction (six term products per product, fp32-grade; what the library uses
 * for products with I, J >= 128 unless MNERF_GEMM_MATH=f32), 0 = the exact-f32 matrix instruction. */
int mnerf_debug_gemm(const float* a, int64_t sa_i, int64_t sa_k, const float* b, int64_t sb_k, int64_t sb_j, float* c,
                     int64_t sc_i, const float* bias, int32_t I, int32_t J, int32_t K, int32_t mode, int32_t math,
                     void* stream);

/* ABI v10 - the tail of a training iteration (coach.py:215-243 of the reference: the L2 loss, clip_grad_norm_ on the encoder and
 * torch.optim.AdamW.step) as streaming kernels over ALL parameter tensors at once (matchnerf_amd/csrc/optim.hip).
 *
 * The tensors travel as a DEVICE table of rows, sorted by group; tensors without a gradient are not rows (torch skips them and does
 * not advance their step).  A tensor is cut into chunks of MNERF_OPTIM_CHUNK elements, one workgroup per chunk: block_begin is the
 * running sum of the rows' chunk counts (row 0: 0), n_blocks the total.  Pointers need 4-byte alignment only; a row whose four
 * pointers are 16-byte aligned takes the vector path. */
#define MNERF_OPTIM_CHUNK 4096
#define MNERF_OPTIM_MAX_GROUPS 8
typedef struct mnerf_optim_row {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  int32_t group;               /* index into the groups array */
  int32_t block_begin;         /* first workgroup of this row */
  double bias_correction1;     /* 1 - beta1^step of THIS tensor, formed on the host in double (lr / it is rounded once) */
  float bias_correction2_sqrt; /* sqrt(1 - beta2^step) */
  int32_t pad_;
} mnerf_optim_row;
/* Hyperparameters of one parameter group, BY VALUE (a host array; nothing is copied to the device but kernel arguments).
 * n_blocks: workgroups of the group's rows.  max_norm <= 0: the group is not clipped. */
typedef struct mnerf_optim_group {
  double lr, beta1, beta2, eps, weight_decay, max_norm;
  int32_t n_blocks;
  int32_t pad_;
} mnerf_optim_group;
/* chunks of a tensor of numel elements (host only; -1 for numel <= 0) */
int64_t mnerf_optim_row_blocks(int64_t numel);
/* sumsq[g] = sum of grad^2 over the rows of group g, for every group.  Deterministic: every workgroup writes the sum of its chunk
 * to workspace[block] (n_blocks floats), one workgroup per group adds them in a fixed order; no floating-point atomics, two calls on
 * the same input give the same bits.  Two launches. */
int mnerf_grad_sumsq(const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks, const mnerf_optim_group* groups,
                     int32_t n_groups, float* workspace, float* sumsq, void* stream);
/* One launch: for every row, with c = min(1, max_norm / (sqrt(sumsq[group]) + 1e-6)) for a clipped group (read on the device) and
 * 1 otherwise, the fp32 chain of torch.optim.AdamW:
 *   grad *= c (written back when c < 1);  param *= 1 - lr weight_decay;  exp_avg += (1 - beta1) (grad - exp_avg);
 *   exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) grad^2;
 *   param -= (lr / bias_correction1) exp_avg / (sqrt(exp_avg_sq) / bias_correction2_sqrt + eps).
 * sumsq: what mnerf_grad_sumsq wrote (may be NULL when no group clips). */
int mnerf_adamw_step(const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks, const mnerf_optim_group* groups,
                     int32_t n_groups, const float* sumsq, void* stream);
/* loss[0] = weight * mean((pred - target)^2) over n elements and, unless grad is NULL, grad[i] = 2 weight (pred[i] - target[i]) / n
 * (coach.py:36-38, 257 and its autograd).  One launch of one workgroup, fixed summation order: bit-reproducible. */
int mnerf_l2_loss(const float* pred, const float* target, int64_t n, float weight, float* loss, float* grad, void* stream);

/* ABI v11 - data-parallel training: the gradients of all rows of the table above as ONE contiguous bucket, so that one collective
 * sums them over the ranks.  Chunk b of the table (b = block_begin of its row + chunk within the row) lies at float offset
 * b * MNERF_OPTIM_CHUNK - every row starts 16-byte aligned whatever its gradient's own alignment -, elements behind numel are
 * zero, and one more chunk of MNERF_OPTIM_CHUNK side slots follows the n_blocks chunks (the iteration's loss rides there).
 * Only grad, numel and block_begin of a row are read.  bucket: 16-byte aligned, mnerf_grad_bucket_floats(n_blocks) floats. */
/* floats of the bucket of a table of n_blocks chunks: (n_blocks + 1) * MNERF_OPTIM_CHUNK (host only; -1 for n_blocks < 1) */
int64_t mnerf_grad_bucket_floats(int64_t n_blocks);
/* One launch: every gradient chunk into its slot, zeros behind numel; side[0, n_side) (device; NULL with n_side 0) into the side
 * chunk, zeros behind it.  n_side <= MNERF_OPTIM_CHUNK. */
int mnerf_grad_pack(const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks, const float* side, int32_t n_side,
                    float* bucket, void* stream);
/* One launch: grad = bucket * scale for every row (one fp32 multiply per element), side_out[0, n_side) = side slots * scale. */
int mnerf_grad_unpack(const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks, const float* bucket, float scale,
                      float* side_out, int32_t n_side, void* stream);

/* ABI v12 - evaluation on the device (misc/metrics.py:19-45 and the per-image host loop of coach.py:316-453 of the reference):
 * PSNR and SSIM of n_images rendered frames against their ground truth, as `psnr` and `EvalTools.set_inputs` + `ssim` of
 * matchnerf_amd/metrics.py compute them with data_range = 2.
 *   pred          [n, H*W, 3] channel-last, contiguous: what the forward pass returns as rgb
 *   gt            [n, 3, H, W] channel-first, image i at gt + i * gt_image_stride (floats; >= 3 H W): the target view of a
 *                 [B, V, 3, H, W] batch passes without a copy
 *   invalid_mask  [n, H, W] bytes, non-zero = the pixel is dropped, or NULL
 * With a mask the mean squared error runs over the three channels of the kept pixels and SSIM over the whole image with the
 * masked pixels set to 0 in both images (H, W >= 7); without one both use the crop [H/10, H - H/10) x [W/10, W - W/10)
 * (H, W >= 10).  SSIM: 7x7 windows that lie inside the processed image, sample covariance (49/48), C1 = 0.02^2, C2 = 0.06^2, mean
 * over windows and channels.  Inputs are fp32; products, sums and the SSIM expression are fp64.
 *   out           [n, 4] doubles: PSNR in dB, SSIM, MSE, kept pixels.  No kept pixel: PSNR and MSE are NaN; MSE 0: PSNR +inf.
 *   workspace     8-byte aligned, at least the bytes the helper below returns
 * Deterministic: every workgroup writes its own workspace slots, one workgroup per image adds them in a fixed order; no
 * floating-point atomics.  The four numbers of an image depend neither on the other images nor on n_images.  Two launches.
 * Sizes below the limits: MNERF_E_RANGE. */
/* host only; -1 for n_images < 1 or H, W < 7 */
int64_t mnerf_image_metrics_workspace_bytes(int32_t n_images, int32_t height, int32_t width);
int mnerf_image_metrics(const float* pred, const float* gt, int64_t gt_image_stride, const uint8_t* invalid_mask,
                        int32_t n_images, int32_t height, int32_t width, void* workspace, double* out, void* stream);

/* ABI v12 (added without a layout change) - LPIPS on the device: the VGG-16 variant of lpips v0.1 as matchnerf_amd/metrics.py
 * (LPIPSVGG) restates it, replacing lpips.LPIPS(net='vgg') of misc/metrics.py:14-17,47-52 of the reference.  Same signature data as
 * mnerf_image_metrics (pred [n, H*W, 3], gt [n, 3, H, W] with an image stride, invalid_mask [n, H, W] bytes or NULL).  With a mask the
 * whole frame is used with the masked pixels set to 0 in both images (in [0, 1] space); without one the crop [H/10, H - H/10) x
 * [W/10, W - W/10).  Then 2x - 1, (x - shift) / scale, the 13 convolutions 3x3 + bias + ReLU through mnerf_conv2d (three-product
 * split-fp16, one power-of-two gain per operand tensor, fp32 accumulation; the first layer reads the 3 channels zero-padded to 32),
 * four 2x2 max-pools and, after each of the five stages, the head: per pixel, unit(a) - unit(b) (channel norm + 1e-10), squared,
 * weighted by the stage's non-negative head vector, spatial mean; the five means are added.  Norms, squares, sums and means are
 * fp64.  The network is walked one pair (pred i, gt i) at a time with the pair's own absmax regions: out[i] depends neither on the
 * other images nor on n_images, two runs are bit-identical (no floating-point atomics), and pred i == gt i gives exactly 0.
 *   weights       the 13 layers in network order (relu1_1 .. relu5_3): wstream[l] = mnerf_lpips_wstream_floats(l) words, 16-byte
 *                 aligned (gmflow.pack_conv_blocks; layer 0 from the weight zero-padded to 32 input channels), bias[l] [c_out],
 *                 ew[l] the stream's exponent; head[s] [64 / 128 / 256 / 512 / 512] floats
 *   workspace     16-byte aligned, mnerf_lpips_workspace_bytes(n, H, W, mask != NULL) bytes: two activation buffers shared by all
 *                 pairs + n x (network input, 14 absmax regions, head slots):  bytes(n) = bytes(1) + (n - 1) x (bytes(2) - bytes(1))
 *   out           [n] doubles, 8-byte aligned
 * Every argument check precedes any launch (MNERF_E_NULL / _RANGE / _ALIGN).  Enqueue only.  The processed image must be at least
 * 16 x 16 (four pools).  The one-gain-per-tensor split has been checked on random and layer-rescaled weights only; parity with the
 * `lpips` package on its real weights is unpinned (tools/eval_time.py prints both paths' values for a user who has the files). */
typedef struct mnerf_lpips_weights {
  const float* wstream[13];
  const float* bias[13];
  const float* head[5];
  int32_t ew[13];
} mnerf_lpips_weights;
/* host only; words of layer's weight stream (0 outside 0..12) */
int64_t mnerf_lpips_wstream_floats(int32_t layer);
/* host only; -1 for n_images < 1 or a processed image below 16 x 16 */
int64_t mnerf_lpips_workspace_bytes(int32_t n_images, int32_t height, int32_t width, int32_t masked);
int mnerf_lpips_vgg(const float* pred, const float* gt, int64_t gt_image_stride, const uint8_t* invalid_mask, int32_t n_images,
                    int32_t height, int32_t width, const mnerf_lpips_weights* weights, void* workspace, double* out, void* stream);
/* The building blocks, exported so that they can be tested alone (the wide convolution: mnerf_conv2d with c_out 256 / 512).
 * mnerf_maxpool2x2: F.max_pool2d(x, 2, 2) of in [planes][h][w] -> out [planes][h/2][w/2] (floor: an odd last row / column is dropped).
 * mnerf_lpips_head: one stage of one pair, feat_a / feat_b [channels][h][w] fp32 -> mnerf_lpips_head_slots(h, w) doubles, one per
 * workgroup of 64 pixels, each already divided by h w; mnerf_lpips_sum: out[i] = the sum of image i's n_slots doubles at
 * slots + i * image_stride, added in a fixed order by one workgroup. */
int mnerf_maxpool2x2(const float* in, float* out, int64_t planes, int32_t h, int32_t w, void* stream);
int64_t mnerf_lpips_head_slots(int32_t h, int32_t w);
int mnerf_lpips_head(const float* feat_a, const float* feat_b, const float* head_w, int32_t channels, int32_t h, int32_t w,
                     double* slots, void* stream);
int mnerf_lpips_sum(const double* slots, int64_t image_stride, int32_t n_slots, int32_t n_images, double* out, void* stream);

/* GEOMETRY EXPORT (added under v12 without a layout change; matchnerf_amd/csrc/fusion.hip): depth maps rendered at several poses of
 * one encoded scene, filtered by cross-view consistency (the MVSNet criterion) and back-projected into one coloured point cloud; and
 * the colour map of the reference's depth panels.  The ray transformer makes a sample's density depend on all samples of its ray, so
 * a density grid has no meaning here; a rendered depth map has.  The geometry is pinhole camera-z depth: what a render returns for
 * pixel rays with depth.param = metric (their camera-z is 1).  Replaces nothing in the reference, which shows depth (coach.py:404-408,
 * 497-505) but exports none.  Enqueue-only on `stream`; every argument check precedes any HIP call; no floating-point atomics and no
 * atomic cursor: two runs give the same bits.  Poses travel as mnerf_view (HOST arrays, read during the call; in the kernel
 * arguments by value): world->camera extr, the intr of THIS height x width grid, near_ / far_ = the valid depth range.  The host
 * inverts intr and extr's [R|t] in double ([R^-1 | -R^-1 t], 3x3 adjugates) and casts to fp32; the device chain is fp32 with the
 * k-ordered FMA products of the projection code:
 *   lift(view, x, y, z)   cam = kinv (x, y, 1) as for pixel rays, each component times z, world = c2w [cam; 1]
 *   proj(view, world)     c = extr [world; 1], q = intr c  ->  (q0 / q2, q1 / q2, q2): pixel coordinates and camera-z
 * Pixel centres are the integer coordinates with legacy_coord and + 0.5 otherwise; pixel index = y * width + x.
 *
 * mnerf_depth_consistency - one thread per pixel p = (x, y) of view `ref`:
 *   depth          device [n_views][height][width] fp32;  opacity: the same shape, or NULL
 *   value of a pixel of view k: z = depth (opacity NULL) or depth / opacity, the normalised expected depth; VALID iff (opacity NULL
 *   or opacity >= min_opacity) and z is finite and views[k].near_ <= z <= views[k].far_
 *   p invalid: n_consistent = 0, fused_depth = 0.  Otherwise P = lift(ref, p, z) and, for every j != ref in ascending order:
 *     (u, v, zj) = proj(j, P); j is skipped if zj <= 0 or (u, v) lies outside the rectangle of view j's pixel centres;
 *     dj = the bilinear value of view j at (u, v): with (fx, fy) = (u, v) - centre offset, x0 = min(floor(fx), width - 2) (0 for a
 *     width of 1), x1 = min(x0 + 1, width - 1), ax = fx - x0, rows alike; the FOUR taps (x0|x1, y0|y1) are normalised by their own
 *     opacities and must all be valid (whatever their weights), else j is skipped; dj = top + ay (bot - top) with
 *     top = z00 + ax (z10 - z00), bot = z01 + ax (z11 - z01), each a + t b one FMA;
 *     (x', y', d') = proj(ref, lift(j, u, v, dj)); j is CONSISTENT iff hypot(x' - x, y' - y) < px_tol and |d' - z| < rel_tol z
 *   n_consistent [height][width] int32 = the number of consistent j; fused_depth [height][width] = (z + sum of their d') / (1 + n),
 *   added in the order of j.
 * MNERF_E_RANGE: n_views outside 2..MNERF_MAX_VIEWS, ref outside the views, height or width below 1 or height x width >= 2^31, a
 * px_tol or rel_tol that is not finite and positive, a min_opacity that is not finite (read only with opacity), a singular intr or
 * extr.  MNERF_E_NULL: views, depth, fused_depth or n_consistent missing. */
int mnerf_depth_consistency(const mnerf_view* views, int32_t n_views, int32_t ref, int32_t height, int32_t width, int32_t legacy_coord,
                            const float* depth, const float* opacity, float px_tol, float rel_tol, float min_opacity,
                            float* fused_depth, int32_t* n_consistent, void* stream);

/* mnerf_point_cloud - the selected pixels of one view as rows of a point buffer, in pixel order (a stable compaction):
 *   selected       n_consistent[i] >= min_consistent and depth[i] finite and > 0 (pass the fused depth)
 *   points         device, rows of 32 bytes, 16-byte aligned (MNERF_E_ALIGN otherwise): x y z d | r g b n - the row size of a ray
 *                  bundle -, xyz = lift(view, pixel centre, depth), d the depth, rgb the pixel's colour from rgb [height x width][3],
 *                  n the count as a float
 *   count          device, one int64: the number of selected pixels.  Rows at or beyond `capacity` are not written and the call is
 *                  still MNERF_OK: a caller sizes one buffer (height x width rows always suffice), copies count once and trims
 *   workspace      device, 4-byte aligned, mnerf_point_cloud_workspace_bytes(height x width) bytes; scratch only
 * Four launches: every workgroup of 256 pixels counts its selected pixels with wave ballots; the counts are scanned in tiles of
 * 1024 by one workgroup each; one workgroup scans the tile totals and writes count; every workgroup writes its rows at its base +
 * the ballot prefix of each pixel.  Integer arithmetic only: the rows and their order are the same bits on every run.
 * height x width == 0 is MNERF_OK and touches no buffer (count included).  MNERF_E_RANGE: a negative size, height x width >= 2^31, a
 * negative capacity, a singular intr or extr.  MNERF_E_NULL: view, depth, rgb, n_consistent, count or workspace missing, or points with
 * capacity > 0.
 * mnerf_point_cloud_workspace_bytes: host only; 4 (ceil(n / 256) + ceil(n / 262144)) rounded up to 16; 0 for 0 pixels, -1 for a
 * negative count. */
int64_t mnerf_point_cloud_workspace_bytes(int64_t n_pixels);
int mnerf_point_cloud(const mnerf_view* view, int32_t height, int32_t width, int32_t legacy_coord, const float* depth, const float* rgb,
                      const int32_t* n_consistent, int32_t min_consistent, float* points, int64_t capacity, int64_t* count,
                      void* workspace, void* stream);

/* mnerf_depth_colormap - depth [n] fp32 -> rgb [n][3] bytes, the arithmetic of visualize_depth (misc/utils.py:323-341) in fp32:
 *   NaN becomes 0;  t = (d - lo) / fp32(hi - lo + 1e-8) (the denominator formed in double);  index = 255 t truncated towards zero and
 *   CLAMPED to 0..255 (anything not above 0 is 0).  numpy's cast to uint8 wraps out-of-range values instead; the clamp is deliberate.
 * then the JET map as a formula, with s = index / 255:
 *   r = clamp(1.5 - |4 s - 3|), g = clamp(1.5 - |4 s - 2|), b = clamp(1.5 - |4 s - 1|) on [0, 1], times 255 and rounded half up -
 *   evaluated exactly in integers: r = clamp(383 - |4 index - 765|, 0, 255), g with 510, b with 255.
 * This is the classic piecewise-linear JET, not OpenCV's 256-entry table (cv2.applyColorMap): parity with that table is unpinned.
 * n == 0 is MNERF_OK and touches no buffer.  MNERF_E_RANGE: n < 0, lo or hi not finite.  MNERF_E_NULL: depth or rgb missing. */
int mnerf_depth_colormap(const float* depth, int64_t n, float lo, float hi, uint8_t* rgb, void* stream);

/* MESH EXPORT (added under v12 without a layout change; matchnerf_amd/csrc/mesh.hip): truncated-signed-distance (TSDF) fusion of the
 * depth maps of GEOMETRY EXPORT into a voxel volume, and a mesher that extracts a welded, indexed, coloured triangle mesh from it.
 * The conventions are those of GEOMETRY EXPORT: pinhole camera-z depth, mnerf_view HOST arrays read during the call, proj() and the
 * value of a texel as stated there, pixel centres by legacy_coord, enqueue-only on `stream`, every argument check before any HIP
 * call, no atomics of any kind, every operation rounded on its own with one FMA where the text says so.
 * The grid: nx x ny x nz voxels of side `voxel` (finite, > 0) from the corner (origin_x, origin_y, origin_z) (finite); voxel
 * (i, j, k) has the linear index (k ny + j) nx + i - x fastest - and the centre origin + (index + 0.5) voxel, one FMA per axis.
 * A grid with nx ny nz == 0 is MNERF_OK and touches no buffer.
 *
 * mnerf_tsdf_integrate - one thread per voxel, one launch; adds n_views (1..MNERF_MAX_VIEWS) depth maps to a volume that the caller
 * owns and has zeroed before the first call:
 *   sums           device [nz][ny][nx][4] fp32, 16-byte aligned (MNERF_E_ALIGN otherwise): S | R G B, the running sums of the
 *                  truncated distance and of the colour
 *   weight         device [nz][ny][nx] fp32: the number of views that updated the voxel
 *   depth          device [n_views][height][width];  opacity: the same shape or NULL;  rgb [n_views][height x width][3]
 *   n_consistent   device [n_views][height][width] int32 or NULL.  With it pass the FUSED depth of mnerf_depth_consistency and
 *                  opacity = NULL; a texel then also needs n_consistent >= min_consistent
 * With P the voxel's centre, for view j in ascending order:
 *   (u, v, zc) = proj(j, P); skipped unless zc > 0;
 *   the nearest texel xi = floor((u - off) + 0.5), yi alike (off = the centre offset); skipped outside 0 <= xi < width, 0 <= yi < height;
 *   z = the texel's value; skipped when it is not VALID (or fails n_consistent);
 *   sdf = z - zc; skipped if sdf < -trunc (the voxel is hidden behind the surface); t = min(1, sdf / trunc);
 *   S += t, RGB += rgb[texel], weight += 1.
 * Calls accumulate: more views are several calls on one volume, and the result depends on the order of the views only.
 * MNERF_E_RANGE: n_views outside 1..MNERF_MAX_VIEWS, height or width below 1 or height x width >= 2^31, trunc not finite and
 * positive, a min_opacity that is not finite (read only with opacity), a grid size below 0, nx ny nz >= 2^31, a voxel not finite and
 * positive, an origin not finite, a singular intr or extr.  MNERF_E_NULL: views, depth, rgb, sums or weight missing.  MNERF_E_ALIGN: sums not
 * 16-byte or weight not 4-byte aligned. */
int mnerf_tsdf_integrate(const mnerf_view* views, int32_t n_views, int32_t height, int32_t width, int32_t legacy_coord,
                         const float* depth, const float* opacity, const int32_t* n_consistent, int32_t min_consistent, const float* rgb,
                         float min_opacity, float trunc, float origin_x, float origin_y, float origin_z, float voxel, int32_t nx,
                         int32_t ny, int32_t nz, float* sums, float* weight, void* stream);

/* mnerf_tsdf_mesh - marching tetrahedra over the Freudenthal split of every cell of the volume's lattice.
 *   lattice        the lattice points are the voxel centres; the value at a point is d = S / weight; a point is VALID iff
 *                  weight >= min_weight (finite, > 0); INSIDE is d < 0 (an exact 0 is outside; the zero-area triangles this can give
 *                  are kept, so that the welded indices stay watertight)
 *   cells          cell (i, j, k), 0 <= i < nx - 1 and alike, has the corners (i, j, k) + c, c in {0,1}^3; it is valid iff its 8
 *                  corners are.  Cells are ordered by (k, j, i), x fastest.  A grid with an axis of 1 has no cell.
 *   tets           a cell's six tets, in this order, are the axis permutations xyz xzy yxz yzx zxy zyx: tet (a b c) has the
 *                  vertices v0 = 000, v1 = e_a, v2 = e_a + e_b, v3 = 111.  The even permutations (tets 0, 3, 4) are positively
 *                  oriented, det[v1 - v0, v2 - v0, v3 - v0] = +1.
 *   edges          every tet edge runs from a lattice point p to p + e, e a non-zero corner of {0,1}^3; p OWNS it under the
 *                  direction index e_x + 2 e_y + 4 e_z - 1 = 0..6: +x, +y, +x+y, +z, +x+z, +y+z, +x+y+z.
 *   vertices       one per owned edge whose ends differ in INSIDE and that at least one valid cell uses (the cells p - f, f a corner
 *                  with f . e = 0).  With a = p, b = p + e:  s = da / (da - db);  position = pa + s (pb - pa), weight and colour
 *                  (RGB / weight of each end) alike, every component one FMA.  A row is 32 bytes: x y z w | r g b 0.
 *                  Order: ascending (owner's linear index, direction index).
 *   triangles      int32 [T][3] vertex rows.  With I the inside and O the outside vertices of a tet, each ascending, and "pq" the
 *                  vertex on the edge between tet vertices p and q:
 *                    |I| = 1, I = {a}, O = {b c d}:   (ab ac ad)
 *                    |I| = 3, O = {a}, I = {b c d}:   (ab ac ad)
 *                    |I| = 2, I = {a b}, O = {c d}:   (ac ad bd) then (ac bd bc) - the quad ac ad bd bc cut along ac-bd
 *                  The last two vertices of every triangle are swapped once if the permutation (I, O) of 0123 is odd and once if
 *                  the tet is: the geometric normal then points from negative to positive d, towards the observed free space.
 *                  Order: ascending (cell, tet, triangle).
 *   vertices       device [vertex_capacity] rows, 16-byte aligned;  triangles: device [triangle_capacity][3] int32
 *   counts         device int64[2], 8-byte aligned: the numbers of vertices and triangles.  Rows at or beyond a capacity are not
 *                  written, the counts are the totals either way and the call is MNERF_OK (as mnerf_point_cloud)
 *   workspace      device, 4-byte aligned, mnerf_tsdf_mesh_workspace_bytes(nx, ny, nz) bytes; scratch only.  With N = nx ny nz,
 *                  B = ceil(N / 256), T = ceil(B / 1024):  int32 vertex base of every lattice point [N] | int32 [B] and [T]: the
 *                  vertex counts of the workgroups and of their tiles, scanned | the same two for the triangles | uint8 flags [N]
 *                  (1 valid, 2 inside, 4 origin of a valid cell) | uint8 masks [N] (bit = direction index of a live owned edge):
 *                  4 (N + 2 B + 2 T) + 2 N bytes, rounded up to 16.
 * Nine launches over the lattice points, 256 per workgroup: flags; edge masks and workgroup counts; the point cloud's two scans;
 * vertex bases and rows; the triangle counts of the cells (a thread is the cell its point is the origin of); two scans; the index
 * triples, each vertex looked up as its owner's base + the popcount of the lower mask bits.  The 16 tet cases are generated from the
 * rule above at compile time.  Integer arithmetic decides every row's place: two runs give the same bytes.
 * MNERF_E_RANGE: a grid size below 0, nx ny nz > (2^31 - 1) / 12 (what keeps 7 vertices per point and 12 triangles per cell below
 * 2^31), a voxel not finite and positive, an origin not finite, min_weight not finite and positive, a negative capacity.
 * MNERF_E_NULL: sums, weight, counts or workspace missing, vertices or triangles missing with a capacity > 0.  MNERF_E_ALIGN: sums or
 * vertices not 16-byte, counts not 8-byte, weight, triangles or workspace not 4-byte aligned.
 * mnerf_tsdf_mesh_workspace_bytes: host only; 0 for an empty grid, -1 for a size below 0 or above the bound. */
int64_t mnerf_tsdf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int mnerf_tsdf_mesh(const float* sums, const float* weight, float origin_x, float origin_y, float origin_z, float voxel, int32_t nx,
                    int32_t ny, int32_t nz, float min_weight, float* vertices, int64_t vertex_capacity, int32_t* triangles,
                    int64_t triangle_capacity, int64_t* counts, void* workspace, void* stream);

/* SPARSE TSDF VOLUME (MESH EXPORT, continued; added under v12 without a layout change; matchnerf_amd/csrc/tsdf_sparse.hip): the same
 * volume and the same mesh, stored only where a surface can be, for grids past what the dense functions take.  The conventions are
 * those of MESH EXPORT.  The grid nx x ny x nz above is VIRTUAL: it is covered by bricks of MNERF_TSDF_BRICK^3 = 8 x 8 x 8 voxels,
 * bx = ceil(nx / 8) per axis and alike, partial bricks at the high faces.
 *   marks          device uint8 [bz][by][bx], x fastest: non-zero = the brick is wanted
 *   table          device int32 [bz][by][bx]: the brick's SLOT, or -1.  Slots ascend with the brick's linear index (k by + j) bx + i
 *   bricks         device int32 [bx by bz]: the first n_bricks entries are the linear indices of the allocated bricks, ascending -
 *                  the table's inverse
 *   sums, weight   device [n_bricks][512][4] and [n_bricks][512] fp32, as in mnerf_tsdf_integrate, zeroed by the caller: voxel
 *                  (i, j, k) of the brick in slot s is point s 512 + ((k & 7) 8 + (j & 7)) 8 + (i & 7).  Voxels of a partial brick
 *                  outside the virtual grid are never updated and are never lattice points.
 * The call order is mark (once per group of views), table, one device->host copy of the count, the caller's allocation,
 * integrate_sparse (once per group), mesh_sparse.  A grid with nx ny nz == 0, or n_bricks == 0, is MNERF_OK and touches no buffer.
 *
 * mnerf_tsdf_bricks_mark - one workgroup per brick of the virtual grid, one thread per two voxels (so no linear voxel index over
 * the virtual grid), one launch per 2^22 bricks.  A voxel is NEAR iff for at least one view mnerf_tsdf_integrate's update of that voxel happens
 * with t < 1: the texel passes every test and -trunc <= sdf, sdf / trunc < 1.  The per-view step is the device function the
 * integrators call, so the mark agrees with them bit for bit.  A NEAR voxel marks the brick of every voxel of its 3 x 3 x 3
 * neighbourhood that lies inside the grid: that keeps every cell a triangle can come from, with the lattice points its vertices
 * interpolate, inside allocated bricks, so the mesh is the dense one (see mnerf_tsdf_mesh_sparse).  The caller zeroes `marks`
 * before the first call; calls OR into it (plain stores of 1, no atomic), which is how views beyond MNERF_MAX_VIEWS are added.
 * MNERF_E_RANGE: as mnerf_tsdf_integrate, with bx by bz >= 2^31 in the place of nx ny nz >= 2^31.  MNERF_E_NULL: views, depth or
 * marks missing. */
#define MNERF_TSDF_BRICK 8
int mnerf_tsdf_bricks_mark(const mnerf_view* views, int32_t n_views, int32_t height, int32_t width, int32_t legacy_coord,
                           const float* depth, const float* opacity, const int32_t* n_consistent, int32_t min_consistent,
                           float min_opacity, float trunc, float origin_x, float origin_y, float origin_z, float voxel, int32_t nx,
                           int32_t ny, int32_t nz, uint8_t* marks, void* stream);

/* mnerf_tsdf_bricks_table - marks -> table, bricks and count (device int64, 8-byte aligned: the number of marked bricks), by a
 * count, the two-level scan and a scatter: four launches, the same bytes on every run.  Takes the BRICK grid (bx, by, bz).
 *   workspace      device, 4-byte aligned, mnerf_tsdf_bricks_table_workspace_bytes(bx, by, bz) bytes: with N = bx by bz,
 *                  B = ceil(N / 256), T = ceil(B / 1024): int32 [B] | int32 [T], 4 (B + T) bytes rounded up to 16
 * With bx by bz == 0 the count, 0, is written all the same.  MNERF_E_RANGE: a size below 0, bx by bz >= 2^31.  MNERF_E_NULL: count
 * missing; marks, table, bricks or workspace missing with bx by bz > 0.  MNERF_E_ALIGN: table, bricks or workspace not 4-byte, count
 * not 8-byte aligned.  mnerf_tsdf_bricks_table_workspace_bytes: host only; -1 beyond the bounds. */
int64_t mnerf_tsdf_bricks_table_workspace_bytes(int32_t bx, int32_t by, int32_t bz);
int mnerf_tsdf_bricks_table(const uint8_t* marks, int32_t bx, int32_t by, int32_t bz, int32_t* table, int32_t* bricks, int64_t* count,
                            void* workspace, void* stream);

/* mnerf_tsdf_integrate_sparse - mnerf_tsdf_integrate on the allocated bricks: one workgroup per brick, the dense update on the
 * voxel's GLOBAL index (centre = origin + (index + 0.5) voxel, one FMA per axis), so every allocated voxel ends with exactly the bits
 * the dense volume has there.  Calls accumulate as the dense ones do.
 * MNERF_E_RANGE: as mnerf_tsdf_bricks_mark; n_bricks below 0, above bx by bz or above 349 525 (see mnerf_tsdf_mesh_sparse).
 * MNERF_E_NULL: views, depth, rgb, bricks, sums or weight missing.  MNERF_E_ALIGN: sums not 16-byte, weight or bricks not 4-byte
 * aligned. */
int mnerf_tsdf_integrate_sparse(const mnerf_view* views, int32_t n_views, int32_t height, int32_t width, int32_t legacy_coord,
                                const float* depth, const float* opacity, const int32_t* n_consistent, int32_t min_consistent,
                                const float* rgb, float min_opacity, float trunc, float origin_x, float origin_y, float origin_z,
                                float voxel, int32_t nx, int32_t ny, int32_t nz, const int32_t* bricks, int64_t n_bricks, float* sums,
                                float* weight, void* stream);

/* mnerf_tsdf_mesh_sparse - mnerf_tsdf_mesh's nine launches over the n_bricks x 512 allocated points.  The neighbour p + e of a point
 * is found through the table: the brick of its global index -> slot -> in-brick index.  A point of a brick without a slot, or
 * outside the virtual grid, is not VALID.  Flags, edge masks, the owner rule, the 16 tet cases, the winding and the behaviour at a
 * capacity (rows beyond it are dropped, the counts stay the totals) are those of mnerf_tsdf_mesh.
 * ORDER: vertices ascend in (slot, in-brick index of the owner, direction index); triangles ascend in (slot of the cell's origin
 * point, in-brick index, tet, triangle).
 * GUARANTEE: with the marks of mnerf_tsdf_bricks_mark for the same views and grid (or any superset of them), the set of vertex rows
 * and the triangles are exactly those of mnerf_tsdf_mesh on the dense volume, bit for bit, under that renumbering.
 *   table, bricks  as mnerf_tsdf_bricks_table left them; table entries must lie in -1 .. n_bricks - 1 (they are not checked)
 *   workspace      device, 4-byte aligned, mnerf_tsdf_mesh_sparse_workspace_bytes(n_bricks, bx, by, bz) bytes: the layout of
 *                  mnerf_tsdf_mesh with N = 512 n_bricks
 * MNERF_E_RANGE: a grid size below 0 (each of nx, ny, nz is an int32, so below 2^31), bx by bz >= 2^31, n_bricks below 0 or above
 * bx by bz, 512 n_bricks > (2^31 - 1) / 12 - that is n_bricks > 349 525, the dense row bound on the allocated points -, a voxel not
 * finite and positive, an origin not finite, min_weight not finite and positive, a negative capacity.  MNERF_E_NULL: sums, weight,
 * table, bricks, counts or workspace missing, vertices or triangles missing with a capacity > 0.  MNERF_E_ALIGN: sums or vertices not
 * 16-byte, counts not 8-byte, weight, triangles, table, bricks or workspace not 4-byte aligned.
 * mnerf_tsdf_mesh_sparse_workspace_bytes: host only; 0 for n_bricks == 0, -1 beyond the bounds. */
int64_t mnerf_tsdf_mesh_sparse_workspace_bytes(int64_t n_bricks, int32_t bx, int32_t by, int32_t bz);
int mnerf_tsdf_mesh_sparse(const float* sums, const float* weight, const int32_t* table, const int32_t* bricks, int64_t n_bricks,
                           float origin_x, float origin_y, float origin_z, float voxel, int32_t nx, int32_t ny, int32_t nz,
                           float min_weight, float* vertices, int64_t vertex_capacity, int32_t* triangles, int64_t triangle_capacity,
                           int64_t* counts, void* workspace, void* stream);

/* MESH FINISHING (MESH EXPORT, continued; added under v12 without a layout change; matchnerf_amd/csrc/mesh_finish.hip): the clean-up
 * between the mesher's raw zero set and a mesh one can use - adjacency, removal of small connected components, Taubin smoothing,
 * vertex normals.  The functions take ANY indexed triangle mesh in the mesher's layout:
 *   vertices       device [V][8] fp32 rows x y z w | r g b 0, 16-byte aligned (MNERF_E_ALIGN otherwise)
 *   triangles      device [T][3] int32 vertex rows, every index in [0, V).  (No kernel reads or writes outside a buffer for an index
 *                  out of that range: such a corner joins no row, such a triangle joins no component and contributes no normal,
 *                  its vertices are boundary vertices, and the compaction drops it.)
 *   0 <= V < 2^31 and 0 <= 3 T < 2^31 (MNERF_E_RANGE otherwise).  V == 0 is MNERF_OK and touches no buffer; T == 0 is the mesh of V
 *   unreferenced vertices (empty rows, no triangle out), and the triangle pointers may then be NULL.
 *   workspace      device, 16-byte aligned, mnerf_mesh_finish_workspace_bytes(V, T) bytes, scratch only; one size serves all calls
 * Enqueue-only on `stream`; every argument check precedes any HIP call (MNERF_E_RANGE, then _NULL, then _ALIGN; int32 buffers are
 * 4-byte aligned).  DETERMINISM: two runs give the same bytes in every output.  No floating-point atomic is used; every float sum
 * runs over a vertex's corners in ascending order inside one thread.  Integer atomics appear only where the final memory contents
 * do not depend on their order: counts (add), the largest component (max), the union-find hooks, and the row fill that is sorted
 * afterwards.  Every operation is rounded on its own, with one FMA where the text says fma().
 *
 * mnerf_mesh_adjacency - the vertex -> corner table in CSR form.  Corner c = 3 t + k is vertex k of triangle t; next(c) and prev(c)
 * are vertices (k + 1) mod 3 and (k + 2) mod 3 of the same triangle.
 *   offsets        device int32 [V + 1], corners: device int32 [3 T].  corners[offsets[v] .. offsets[v + 1]) lists, ASCENDING, the
 *                  corners c with triangles[c] == v.
 *   vertex_class   device uint8 [V]: 1 INTERIOR - the row is not empty and every neighbour (every next and prev vertex of the row's
 *                  corners) is the next vertex of exactly one corner of the row and the prev vertex of exactly one; 0 BOUNDARY -
 *                  everything else: open borders, non-manifold fans, unreferenced vertices.
 * Eight launches: the corner counts (integer atomic add), the mesher's two-level scan over the vertices, the rows filled through an
 * integer cursor, one thread per vertex sorting its own row in place (insertion sort, any length) and classifying it.
 * MNERF_E_NULL: offsets, vertex_class or workspace missing; triangles or corners missing with T > 0.
 *
 * mnerf_mesh_components - connected components (two vertices are connected when a triangle contains both; an unreferenced vertex is
 * a component of its own) by a lock-free union-find over the edges (v0 v1) and (v0 v2) of every triangle: the larger root is hooked
 * under the smaller with a compare-and-swap, a second launch flattens.  No host loop and no copy.
 *   labels         device int32 [V]: the smallest vertex row of the vertex's component
 *   keep           device uint8 [V]: 1 iff the component's triangle count n (triangles counted at the label of their first vertex)
 *                  satisfies n >= min_triangles AND (double) n >= min_fraction * (double) largest, largest = the largest count
 * MNERF_E_RANGE also: min_triangles < 0, min_fraction not finite or outside [0, 1].  MNERF_E_NULL: labels, keep or workspace missing;
 * triangles missing with T > 0.
 *
 * mnerf_mesh_compact - the mesh of the kept vertices.  A triangle is kept iff its FIRST vertex is (all three share a component).
 *   vertices_out   device [vertex_capacity] rows, 16-byte aligned: the kept rows, bit for bit, in their original order
 *   triangles_out  device [triangle_capacity][3] int32: the kept triangles in their original order, indices re-numbered (-1 for
 *                  a vertex that is not kept - none where keep is constant on every component, as mnerf_mesh_components writes it)
 *   counts         device int64 [2], 8-byte aligned: kept vertices, kept triangles.  Rows at or beyond a capacity are not written,
 *                  the counts are the totals either way and the call is MNERF_OK (as mnerf_tsdf_mesh)
 * The mesher's count / scan / scatter, once over the vertices and once over the triangles; no atomics.  The outputs must not
 * overlap the inputs.  MNERF_E_RANGE also: a negative capacity.  MNERF_E_NULL: vertices, keep, counts or workspace missing; triangles
 * missing with T > 0; an output missing with its capacity > 0 (triangles_out only with T > 0).
 *
 * mnerf_mesh_smooth - `iterations` rounds of Taubin smoothing; a round is two Jacobi steps, p <- p + lambda L(p), then
 * p <- p + mu L(p), each one launch of one thread per vertex that reads all positions of the previous step.  For an INTERIOR vertex
 * with the row c_1 < ... < c_n:   s = 0;  s = s + (p[next(c_i)] + p[prev(c_i)]) for i = 1..n, per component;  m = s / (float)(2 n);
 * p' = fma(factor, m - p, p).  That is the uniform umbrella operator: every neighbour of an interior vertex occurs twice.  BOUNDARY
 * vertices do not move (an open border would creep inwards).  Only x y z change: w | r g b 0 are copied bit for bit.
 *   offsets, corners, vertex_class    as mnerf_mesh_adjacency wrote them for THIS mesh
 *   vertices_out   may be vertices_in: the steps ping-pong through the workspace.  iterations == 0: the bytes of vertices_in.
 *                  mu == 0 is plain Laplacian smoothing (the second step copies).
 * MNERF_E_RANGE also: iterations < 0, lambda not in (0, 1], mu not finite or > 0.  MNERF_E_NULL: vertices_in, vertices_out, offsets,
 * vertex_class or workspace missing; triangles or corners missing with T > 0.
 *
 * mnerf_mesh_normals - area-weighted vertex normals, one thread per vertex.
 *   normals        device [V][4] fp32, 16-byte aligned: nx ny nz a.  For the row's corners in ascending order, with (p0, p1, p2) the
 *                  corner's triangle in its stored winding:  u = p1 - p0, v = p2 - p0;  c = u x v with every component
 *                  fma(u_a, v_b, -(u_b v_a)) (x: a b = y z, y: z x, z: x y);  S = S + c;  A = A + |c|,
 *                  |c| = sqrt(fma(c_z, c_z, fma(c_y, c_y, c_x c_x))).  n = S / |S| per component, or 0 0 0 where |S| is not > 0 (an
 *                  unreferenced vertex, zero-area triangles only) - never a NaN for finite input.  a = A / 6: one third of the
 *                  incident area.  On the mesher's output n points towards the observed free space.
 * MNERF_E_NULL: vertices, offsets or normals missing; triangles or corners missing with T > 0.
 *
 * mnerf_mesh_finish_workspace_bytes: host only; -1 beyond the bounds above, 0 for V == 0.  With Bv = ceil(V / 256),
 * Tv = ceil(Bv / 1024) and Bt, Tt alike from T, the workspace is 16 bytes (int64 [2]: the scans' totals / the largest component)
 * followed by the larger of
 *   int32 [V] (adjacency: the fill cursor; components: the triangle counts; compact: the new vertex rows) | int32 [Bv] | [Tv]: the
 *   vertex scan's workgroup and tile counts | int32 [Bt] | [Tt]: the same for the triangle scan        4 (V + Bv + Tv + Bt + Tt) bytes
 *   fp32 [V][8] (smooth: the intermediate positions)                                                     32 V bytes
 * rounded up to 16. */
int64_t mnerf_mesh_finish_workspace_bytes(int64_t n_vertices, int64_t n_triangles);
int mnerf_mesh_adjacency(const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, int32_t* offsets, int32_t* corners,
                         uint8_t* vertex_class, void* workspace, void* stream);
int mnerf_mesh_components(const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, int64_t min_triangles, double min_fraction,
                          int32_t* labels, uint8_t* keep, void* workspace, void* stream);
int mnerf_mesh_compact(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, const uint8_t* keep,
                       float* vertices_out, int64_t vertex_capacity, int32_t* triangles_out, int64_t triangle_capacity, int64_t* counts,
                       void* workspace, void* stream);
int mnerf_mesh_smooth(const float* vertices_in, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const int32_t* offsets,
                      const int32_t* corners, const uint8_t* vertex_class, int32_t iterations, float lambda, float mu,
                      float* vertices_out, void* workspace, void* stream);
int mnerf_mesh_normals(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const int32_t* offsets,
                       const int32_t* corners, float* normals, void* stream);

/* mnerf_mesh_decimate (MESH FINISHING, continued; added under v12 without a layout change; the same file) - decimation by vertex
 * clustering with quadric-error representatives (Lindstrom): the vertices of every cell of a uniform grid become ONE vertex, placed
 * where the squared distances to the planes of the cell's triangles are smallest, and the triangles that still join three different
 * cells are kept once each.  The conventions of the section apply: any [V][8] / [T][3] mesh, the bounds on V and T, V == 0 is
 * MNERF_OK and touches no buffer, enqueue-only, every check before any HIP call (RANGE, NULL, ALIGN), the determinism rule - no
 * floating-point atomic; integer atomics only in the counts of the two CSR tables and in their row fills, the first of which is
 * sorted afterwards and the second of which is only searched for the existence of an entry.  The outputs must not overlap the inputs.
 *   grid           gx x gy x gz cells of side `cell` (finite, > 0) from the corner `origin` (finite); every g* >= 1 and
 *                  gx gy gz < 2^31.  Cell (i, j, k) has the linear index (k gy + j) gx + i.  The grid is DENSE, as the TSDF volume is:
 *                  the workspace holds two int32 per cell, occupied or not
 *   cell of a vertex   per axis q = (x - origin_x) / cell in fp32, the subtraction and the division each rounded on their own;
 *                  i = clamp(floor(q), 0, gx - 1) (a q of +-inf included).  A vertex outside the grid belongs to the nearest border
 *                  cell.  A vertex with a non-finite x, y or z has NO cell: it is dropped, vertex_map[v] = -1
 *   new vertices   one per occupied cell, in ascending linear cell index;  vertex_map: device int32 [V] or NULL, the new row of v's cell
 *   members        a cell's vertices in ascending row order (a cell -> vertex CSR built as mnerf_mesh_adjacency builds its rows:
 *                  integer atomic add, the two-level scan over the cells, the fill through a cursor, the cell's thread sorts its row)
 *   offsets, corners   as mnerf_mesh_adjacency wrote them for THIS mesh (vertex_class is not read)
 *   representative all in fp64, every operation rounded on its own (no FMA).  g = origin + (index + 0.5) cell per axis, evaluated
 *                  in double from the fp32 arguments; every point below is (double) p - g.
 *                  Vertex quadric: for member v, over its corners ascending, the corner's triangle (p0, p1, p2) in stored winding:
 *                    u = p1 - p0, t = p2 - p0;  n = u x t (x: u_y t_z - u_z t_y, y: u_z t_x - u_x t_z, z: u_x t_y - u_y t_x);
 *                    d = -((n_x p0_x + n_y p0_y) + n_z p0_z);  A_v += n n^T (xx xy xz yy yz zz);  b_v += d n.
 *                  n n^T weighs a plane by its squared area: a degenerate triangle adds exactly 0, there is no square root and
 *                  no division.  A triangle with an index outside [0, V) or a non-finite vertex is skipped.
 *                  Cell quadric: A = sum A_v, b = sum b_v over the members ascending.  Means: m = (sum ((double) p_v - g)) / count,
 *                  and w, r, g, b = (sum (double) value) / count, over the members ascending.
 *                  lambda = REG (A_xx + A_yy + A_zz), REG = 1.0 / MNERF_DECIMATE_REG_INV = 1e-3 (the nearest double; the constant is
 *                  kept as its integer inverse because every #define of this header is an integer).  If lambda is not > 0 (no
 *                  area at all): x = m.  Otherwise x solves
 *                  (A + lambda I) x = lambda m - b - symmetric positive definite, condition number <= 1 / REG + 1 - by Gaussian
 *                  elimination without pivoting.  x is then CLAMPED per component to [-cell / 2, +cell / 2] in double (a clamp, not a
 *                  fallback: the result is continuous in its inputs; a NaN goes to the lower bound).
 *                  Row: (float) (g + x) | (float) w | (float) r g b | 0.
 *                  GUARANTEE: every new vertex lies in the closed box g +- cell / 2 of its cell, up to the final rounding to fp32.
 *   triangles      a triangle is a CANDIDATE iff its three indices are in [0, V), its three vertices have cells and its three new
 *                  rows are pairwise distinct; a candidate is KEPT iff no candidate with a smaller triangle index has the same SET
 *                  of three new rows (winding ignored).  triangles_out: the kept triangles in their original order, each with its
 *                  own stored winding, re-numbered.  (The candidates' adjacency over the new rows, by the kernels of
 *                  mnerf_mesh_adjacency; one thread per candidate walks the row of its smallest new row for an earlier triangle
 *                  of the same set; the mesher's count / scan / scatter over the flags.)
 *   vertices_out   device [vertex_capacity] rows, 16-byte aligned;  triangles_out: device [triangle_capacity][3] int32
 *   counts         device int64 [2], 8-byte aligned: new vertices, kept triangles.  Rows at or beyond a capacity are not written,
 *                  the counts are the totals either way and the call is MNERF_OK.  V and T are upper bounds of the two counts.
 *   workspace      device, 16-byte aligned, mnerf_mesh_decimate_workspace_bytes(V, T, gx, gy, gz) bytes, scratch only.  With
 *                  N = gx gy gz, Bn = ceil(N / 256), Tn = ceil(Bn / 1024) and Bv, Tv, Bt, Tt alike from V and T:  int64 [2] |
 *                  int32 [V] the cell of a vertex | [V] the members | [N + 1] the cells' offsets | [N] the fill cursor, then the
 *                  cells' new rows | [Bn] [Tn] | [3 T] the candidates | [V + 1] [V] [3 T] their offsets, cursor and corners |
 *                  [Bv] [Tv] | [Bt] [Tt] | uint8 [T] the kept flags:
 *                  16 + 4 (4 V + 2 N + 2 + 6 T + Bn + Tn + Bv + Tv + Bt + Tt) + T bytes, rounded up to 16.
 * One thread per vertex, cell or triangle, 256 per workgroup; 12 launches for the vertices (11 without vertex_map) and 12 for the
 * triangles (1 with T == 0).  A cell's sums run inside ONE thread: a pathological grid - one cell holding a huge mesh - serialises
 * them (the row is sorted by a heap sort, so that costs n log n, and the sums n).
 * MNERF_E_RANGE: the bounds of the section, a g* < 1, gx gy gz >= 2^31, a cell not finite and positive, an origin not finite, a negative
 * capacity.  MNERF_E_NULL: vertices, offsets, counts or workspace missing; triangles or corners missing with T > 0; an output missing
 * with its capacity > 0.  MNERF_E_ALIGN: vertices, vertices_out or workspace not 16-byte, counts not 8-byte, any other not 4-byte
 * aligned.  mnerf_mesh_decimate_workspace_bytes: host only; -1 beyond the bounds (of V, T or the grid), 0 for V == 0. */
#define MNERF_DECIMATE_REG_INV 1000 /* the regularisation weight of mnerf_mesh_decimate is 1.0 / this */
int64_t mnerf_mesh_decimate_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int32_t gx, int32_t gy, int32_t gz);
int mnerf_mesh_decimate(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, const int32_t* offsets,
                        const int32_t* corners, float origin_x, float origin_y, float origin_z, float cell, int32_t gx, int32_t gy,
                        int32_t gz, float* vertices_out, int64_t vertex_capacity, int32_t* triangles_out, int64_t triangle_capacity,
                        int32_t* vertex_map, int64_t* counts, void* workspace, void* stream);

/* MESH TEXTURE (added under v12 without a layout change; matchnerf_amd/csrc/mesh_texture.hip): a texture atlas for an indexed mesh,
 * baked from the views the mesh was fused from.  The mesh's own colour is one nearest texel per voxel, interpolated and - after a
 * decimation - averaged over a cell; the atlas carries the frames' detail onto the surface.  The conventions are those of GEOMETRY
 * EXPORT and MESH EXPORT: pinhole camera-z depth, mnerf_view HOST arrays read during the call (by value in the kernel arguments),
 * proj(), the VALID test of a texel and the bilinear taps as stated there, pixel centres by legacy_coord, fp32 with every operation
 * rounded on its own and one FMA where the text says fma(), enqueue-only on `stream`, nothing allocated or copied, every argument
 * check before any HIP call (MNERF_E_RANGE, then _NULL, then _ALIGN), no kernel reads or writes outside a buffer for any index
 * value, no atomic of any kind: the only sums run over the views inside one thread, in ascending order, and two runs give the same
 * bytes.  The mesh is any [V][8] / [T][3] mesh of MESH FINISHING with 0 <= V < 2^31, 0 <= 3 T < 2^31; T == 0 is MNERF_OK and touches
 * no buffer.
 *
 * THE ATLAS is a function of (T, block) only, so its size costs no device->host copy.  Every triangle gets a right-triangle patch;
 * two triangles share one square block of B x B texels, B = `block`, 4 <= B <= 64.
 *   nb = ceil(T / 2) blocks;  nbx = the smallest integer with nbx^2 >= nb;  nby = ceil(nb / nbx) (0 for T == 0);  the atlas is
 *   W = nbx B wide and H = nby B high; W or H above 16384 is MNERF_E_RANGE.  Row 0 is the TOP row; texel (x, y) has the linear index
 *   y W + x and its centre at (x + 0.5, y + 0.5).  Block p sits at (p mod nbx, p / nbx); triangle 2 p is its LOWER triangle and
 *   2 p + 1 its UPPER.
 *   corners        in texel units from the block's top-left corner, for the vertices 0, 1, 2 in stored winding:
 *                    lower   (0.5, 0.5), (B - 2.5, 0.5), (0.5, B - 2.5)
 *                    upper   (B - 0.5, B - 0.5), (2.5, B - 0.5), (B - 0.5, 2.5) - the point reflection of the lower
 *   ownership      the local texel (i, j) of a block belongs to the lower triangle iff i + j <= B - 1 and to the upper one
 *                  otherwise; the upper triangle then uses i' = B - 1 - i, j' = B - 1 - j in place of i, j.  A texel has NO OWNER
 *                  when its triangle's index is >= T (a block >= nb; the upper half of the last block when T is odd).
 *   surface        a = i / (B - 3), b = j / (B - 3) (the integers converted, one division each); if s = a + b > 1 then a = a / s,
 *                  b = b / s - the two texel rows past the hypotenuse are clamped onto it.  A quantity q of the vertices is
 *                  blended as fma(b, q2 - q0, fma(a, q1 - q0, q0)); the surface point P is that blend of x, y, z.
 *   GUARANTEE      the corners fall on texel centres, every texel of a block has exactly one owner, and a bilinear fetch anywhere
 *                  inside a triangle's UV triangle gives non-zero weight only to texels that triangle owns: the lower triangle's
 *                  fetches touch texels with i + j <= B - 2 only (the row i + j = B - 1 is a spare for a renderer's rounding), the
 *                  upper triangle's their reflections, i + j >= B.  No gutter pass and no dilation are needed.  (Blocks are not mip-safe across their borders.)
 *   VALID triangle its three indices lie in [0, V), its three positions are finite, and n = (p1 - p0) x (p2 - p0), in the fma form
 *                  of mnerf_mesh_normals, has |n| = sqrt(fma(n_z, n_z, fma(n_y, n_y, n_x n_x))) > 0.
 *
 * mnerf_mesh_texture_atlas - host only: size[0] = W, size[1] = H (a HOST array).  MNERF_E_RANGE: T < 0 or 3 T >= 2^31, block outside
 * 4..64, a side above 16384.  MNERF_E_NULL: size missing.
 *
 * mnerf_mesh_texture_uv - one thread per triangle: uv device [T][3][2] fp32, (x / W, y / H) of the corners with the origin at the
 * top-left.  The numerators (block origin + corner) are half-integers, exact in fp32; one division each.  MNERF_E_RANGE as above;
 * MNERF_E_NULL: uv missing; MNERF_E_ALIGN: uv not 4-byte aligned.
 *
 * mnerf_mesh_texture_accumulate - one thread per texel, one launch; adds n_views (1..MNERF_MAX_VIEWS) views to an accumulation
 * buffer that the caller owns and has zeroed before the first call.  More views are several calls on one buffer, as with the volume.
 *   accum          device [H][W][4] fp32, 16-byte aligned: r g b | w
 *   depth, opacity, n_consistent, min_consistent, rgb, min_opacity    as in mnerf_tsdf_integrate (with n_consistent pass the FUSED
 *                  depth and opacity = NULL)
 * A texel without an owner, or whose triangle is not VALID, is not touched.  Otherwise, with P its surface point and n, |n| its
 * triangle's, for view k in ascending order:
 *   c = the camera centre, the translation column of the host-inverted extr;  e = c - P;  |e| as |n|;
 *   cos = fma(n_z, e_z, fma(n_y, e_y, n_x e_x)) / (|n| |e|); skipped unless cos > 0 (the view looks at the back);
 *   (u, v, zc) = proj(k, P); skipped unless zc > 0 and (u, v) lies in the rectangle of view k's pixel centres;
 *   the four taps of mnerf_depth_consistency at (u, v) must all be VALID - and, with n_consistent, have n_consistent >=
 *   min_consistent - else skipped; d = their bilinear value in the a + t b form;
 *   skipped unless |d - zc| <= vis_rel_tol zc: P is the surface this view sees, not something behind it;
 *   colour = the bilinear value of rgb at the same taps and weights, per channel, in the same form;
 *   weight = 1 multiplied `power` times by cos (an integer 0..8; no powf);
 *   best == 0:  rgb = fma(weight, colour, rgb) per channel, w = w + weight
 *   best != 0:  iff weight > w the texel becomes colour | weight (ties go to the earlier view)
 * MNERF_E_RANGE: the bounds of the mesh and the atlas, n_views outside 1..MNERF_MAX_VIEWS, height or width below 1 or height x width
 * >= 2^31, a min_opacity that is not finite (read only with opacity), vis_rel_tol not finite and positive, power outside 0..8, a
 * singular intr or extr.  MNERF_E_NULL: vertices (with V > 0), triangles, views, depth, rgb or accum missing.  MNERF_E_ALIGN: vertices
 * or accum not 16-byte, any other pointer not 4-byte aligned.
 *
 * mnerf_mesh_texture_resolve - one thread per texel: atlas device [H][W][4] fp32 r g b a, 16-byte aligned; it may be `accum` itself.
 *   an owned texel of a VALID triangle with w > 0:  rgb = sums / w, one division per channel (best == 0) or the stored colour
 *                  (best != 0);  a = 1
 *   the same with w not > 0:  rgb = the blend (see "surface") of the three VERTEX colours, a = 0 - where no view sees the surface
 *                  the atlas shows exactly what the untextured mesh shows
 *   every other texel (no owner, a triangle that is not VALID):  0 0 0 0
 * The atlas is therefore total.  MNERF_E_RANGE: the bounds of the mesh and the atlas.  MNERF_E_NULL: vertices (with V > 0), triangles,
 * accum or atlas missing.  MNERF_E_ALIGN: vertices, accum or atlas not 16-byte, triangles not 4-byte aligned.
 *
 * Texel density is per triangle, not per area: uniform on the mesher's and the decimator's output, wasteful on a mesh of very
 * unequal triangles.  There is no seam levelling between views. */
int mnerf_mesh_texture_atlas(int64_t n_triangles, int32_t block, int32_t* size);
int mnerf_mesh_texture_uv(int64_t n_triangles, int32_t block, float* uv, void* stream);
int mnerf_mesh_texture_accumulate(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, int32_t block,
                                  const mnerf_view* views, int32_t n_views, int32_t height, int32_t width, int32_t legacy_coord,
                                  const float* depth, const float* opacity, const int32_t* n_consistent, int32_t min_consistent,
                                  const float* rgb, float min_opacity, float vis_rel_tol, int32_t power, int32_t best, float* accum,
                                  void* stream);
int mnerf_mesh_texture_resolve(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, int32_t block,
                               int32_t best, const float* accum, float* atlas, void* stream);

/* MESH RASTER (added under v12 without a layout change; matchnerf_amd/csrc/mesh_raster.hip): the indexed mesh seen from one pinhole
 * camera - which triangle every pixel sees, at which depth and where on it - and the shading of that frame from the vertex colours or
 * from the atlas of MESH TEXTURE.  It is what a report on the mesh, a preview and the texture's visibility test against the mesh
 * itself are built from.  The conventions are those of MESH TEXTURE: pinhole camera-z depth, ONE mnerf_view HOST struct read during
 * the call (by value in the kernel arguments), proj() and the pixel centres by legacy_coord as stated under GEOMETRY EXPORT, fp32
 * with every operation rounded on its own and one FMA where the text says fma(), enqueue-only on `stream`, nothing allocated or
 * copied, every argument check before any HIP call (MNERF_E_RANGE, then _NULL, then _ALIGN), no kernel reads or writes outside a
 * buffer for ANY index value in `triangles`.  The mesh is any [V][8] / [T][3] mesh with 0 <= V < 2^31, 0 <= 3 T < 2^31; T == 0 is
 * MNERF_OK and yields the empty frame.  Two runs give the same bytes.
 *
 * DETERMINISM.  The raster uses ONE kind of atomic, a 64-bit UNSIGNED INTEGER minimum, where the texture kernels use none.  The key
 * of a covered pixel is (bits(z) << 32) | triangle: the bits of a positive float are monotone in its value, so keys order by depth
 * and then by triangle index, and equal depths go to the lower index.  The minimum of a set of integers does not depend on the order
 * in which its members arrive, so the key a pixel ends with is a function of the mesh and the camera alone.  No floating-point
 * atomic, no scan, no expansion of work.
 *
 * A triangle is DROPPED unless its three indices lie in [0, V), its three positions are finite, and (u_k, v_k, z_k) = proj(view,
 * p_k) are finite with z_k > 0 for k = 0, 1, 2.  LIMITATION: a triangle that crosses the camera plane is dropped, not clipped.
 *
 * COVERAGE of the pixel centre P = (px, py) = (x, y) + (0 with legacy_coord, 0.5 otherwise), two-sided (front and back faces both
 * cover).  Edge k runs from vertex a = (k + 1) mod 3 to vertex b = (k + 2) mod 3, opposite vertex k.  For an edge a -> b:
 *   swap = u_b < u_a or (u_b == u_a and v_b < v_a);  F = the first endpoint in that (u, then v) order, S = the other
 *   dx = u_S - u_F;  dy = v_S - v_F;  e = fma(dx, py - v_F, -(dy * (px - u_F)));  e = 0 when P equals F or S bit for bit (at S the
 *   fma would leave the rounding error of dy * dx);  value(a -> b, P) = -e with swap, e without
 * so two triangles that traverse one edge in opposite directions get bitwise opposite values at every pixel, whatever the rounding.
 *   area = value(1 -> 2, (u_0, v_0));  area == 0 (or a NaN): no coverage;  s = +1 for area > 0, -1 otherwise
 *   E_k = s * value(a -> b, P);  the gradient of E_k is (gx, gy) = s * (-dy, dx) without swap, s * (dy, -dx) with it (signs only)
 *   the triangle OWNS edge k iff gx > 0, or gx == 0 and gy > 0: its interior lies on the +x side of the edge, or the edge is
 *   horizontal and the interior lies on the +y side - the top-left rule
 *   P is covered iff for k = 0, 1, 2: E_k > 0, or E_k == 0 and the triangle owns edge k
 *   sum = (E_0 + E_1) + E_2, and the pixel is not covered unless sum > 0;  l_k = E_k / sum;  q_k = l_k / z_k;  w = (q_0 + q_1) + q_2;
 *   z = 1 / w;  b_1 = q_1 / w;  b_2 = q_2 / w - perspective-correct weights of the vertices 1 and 2
 * GUARANTEE: a pixel centre on an edge or a vertex shared by triangles on both sides is covered by exactly one of them; a welded
 * closed mesh has neither pinholes nor doubly claimed centres along its edges.
 *
 * mnerf_mesh_raster - three launches on a workspace of uint64 [height][width] keys, 8-byte aligned, mnerf_mesh_raster_workspace_bytes
 * (host only: 8 height width; -1 for a side below 1 or height x width >= 2^31):
 *   clear          one thread per pixel: the key becomes all ones
 *   raster         one wave64 per triangle, four triangles per workgroup of 256: the wave projects the vertices, drops the triangle
 *                  as above, and walks the 8 x 8-pixel blocks (aligned to multiples of 8) that meet the pixels from
 *                  floor(min u - offset) - 1 to ceil(max u - offset) + 1, rows alike, clamped to the frame, lane = pixel.  A covered
 *                  pixel with z > 0 and view.near_ <= z <= view.far_ issues one atomic minimum of its key
 *   resolve        one thread per pixel: the winner's coverage quantities recomputed by the same arithmetic
 *   face           device int32 [height][width]: the triangle, -1 where nothing was hit
 *   depth          device fp32 [height][width]: z, 0 where nothing was hit - not VALID for any consumer with near_ > 0
 *   bary           device fp32 [height][width][2]: (b_1, b_2), 0 where nothing was hit
 * MNERF_E_RANGE: the bounds of the mesh, a side below 1 or height x width >= 2^31, workspace_bytes below the need, a singular intr or
 * extr.  MNERF_E_NULL: view, face, depth, bary or workspace missing; with T > 0 triangles or (with V > 0) vertices missing.
 * MNERF_E_ALIGN: vertices not 16-byte, workspace not 8-byte, any other pointer not 4-byte aligned.
 *
 * mnerf_mesh_shade - one thread per pixel of a rastered frame (face, bary as written above; a face outside [0, T) or with an index
 * outside [0, V) is no hit):
 *   rgba           device fp32 [height][width][4], 16-byte aligned: a = 1 on a hit, 0 0 0 0 elsewhere
 *   atlas == NULL  rgb = fma(b_2, q2 - q0, fma(b_1, q1 - q0, q0)) per channel of the three VERTEX colours (block and the atlas sides
 *                  are not read)
 *   atlas          device fp32 [atlas_height][atlas_width][4], 16-byte aligned, the sides of mnerf_mesh_texture_atlas(T, block): the
 *                  corners' texel coordinates (block origin + corner, the numerators of mnerf_mesh_texture_uv) are blended by
 *                  (b_1, b_2) in the same fma form, per coordinate; rgb = the bilinear value at that point with texel centres at
 *                  + 0.5: the taps and weights of mnerf_depth_consistency over the atlas (x0 = max(min(floor(fx), W - 2), 0), ...),
 *                  top + ay (bot - top) in the a + t b form.  A tap of weight zero is not read (x1 = x0 where ax == 0, rows alike),
 *                  and a tap the triangle does not own is read at the innermost tap instead - (x0, y0) for a lower triangle,
 *                  (x1, y1) for an upper one; only rounding puts a tap there, with a weight below 1e-5.  The rgb therefore depends on
 *                  the triangle's own texels alone (the atlas GUARANTEE)
 *   normal         NULL, or device fp32 [height][width][4], 16-byte aligned: n = (p1 - p0) x (p2 - p0) in the fma form of
 *                  mnerf_mesh_normals, divided by |n| = sqrt(fma(n_z, n_z, fma(n_y, n_y, n_x n_x))) per component, negated when
 *                  fma(n_z, e_z, fma(n_y, e_y, n_x e_x)) < 0 for e = the camera centre (the translation column of the host-inverted
 *                  extr) - p0;  the fourth float is 0;  0 0 0 0 where there is no hit or |n| is not positive and finite
 * MNERF_E_RANGE: the bounds of the mesh, a side below 1 or height x width >= 2^31, with an atlas a block outside 4..64 or sides above
 * 16384 or other than mnerf_mesh_texture_atlas(T, block), a singular intr or extr.  MNERF_E_NULL: view, face, bary or rgba missing;
 * with T > 0 triangles or (with V > 0) vertices missing.  MNERF_E_ALIGN: vertices, atlas, rgba or normal not 16-byte, any other
 * pointer not 4-byte aligned.
 *
 * One wave walks all blocks of its triangle: a triangle that fills the frame costs height x width / 64 steps of one wave.  There is
 * no anti-aliasing and no mip-mapping. */
int64_t mnerf_mesh_raster_workspace_bytes(int32_t height, int32_t width);
int mnerf_mesh_raster(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, const mnerf_view* view,
                      int32_t height, int32_t width, int32_t legacy_coord, int32_t* face, float* depth, float* bary, void* workspace,
                      int64_t workspace_bytes, void* stream);
int mnerf_mesh_shade(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, const int32_t* face,
                     const float* bary, int32_t height, int32_t width, const float* atlas, int32_t atlas_height, int32_t atlas_width,
                     int32_t block, const mnerf_view* view, float* rgba, float* normal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MNERF_H_ */
