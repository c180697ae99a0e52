// Caller-supplied rays (include/mnerf.h "CALLER-SUPPLIED RAYS"): the camera models that fill a ray bundle on the device, the
// per-sample geometry of a bundle, and the render chunk over a bundle.
//
// The radiance field does not care where a ray comes from: every stage after the RayGeom works on world points.  The pixel entry
// points rebuild the ray in-kernel from a pinhole pixel (make_ray, common.hpp); here the ray is a 32-byte row of a buffer, and the
// chunk is staged through the workspace so that the shipped decoder kernel runs unchanged on caller-supplied geometry
// (mnerf_decoder_samples):
//   mnerf_cost_volume_rays (cost_volume.hip: the segment walk, RayGeom from the bundle)  -> cond
//   free_ray_samples_kernel                                                              -> x_ndc, dir, depth_s, ray_len
//   mnerf_decoder_samples                                                                -> rgb_s, sigma
//   mnerf_composite                                                                      -> rgb, depth, opacity
// The staging areas cost 11 floats per sample written once and read once (x_ndc 3, dir 3, depth 1, rgb_s 3, sigma 1): memory-bound
// kernels of a few loads and stores per thread, consecutive threads on consecutive samples / pixels.
#include "common.hpp"

// every expression of this file rounds each operation on its own (the helpers of common.hpp are written for that): the pinhole
// rows are the bits of make_ray, the sample coordinates the bits of ray_samples_kernel
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------ camera models
__device__ __forceinline__ float cam_sin(float radians, int quarter) {  // sin (0) / cos (1), the angle reduced in revolutions
  float th, tl;
  turns_two_float(radians, th, tl);
  return sin_quarter_turns(th, tl, quarter);
}

__global__ __launch_bounds__(256) void camera_rays_kernel(mnerf_camera cam, int pixel_begin, int n_pixels,
                                                          float* __restrict__ ray_od) {
  const long long i64 = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // (n_pixels may lie within a block of 2^31)
  if (i64 >= n_pixels) return;
  const int i = (int)i64;
  float ox, oy, oz, dx, dy, dz;
  if (cam.model == MNERF_CAM_PINHOLE) {  // make_ray itself on the camera's constants
    mnerf_rays R;
    R.ray_idx = nullptr;
    R.ray_begin = pixel_begin;
    R.tgt_width = cam.width;
    R.legacy_coord = cam.legacy_coord;
#pragma unroll
    for (int k = 0; k < 9; ++k) R.kinv[k] = cam.kinv[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) R.c2w[k] = cam.c2w[k];
    const RayGeom g = make_ray(R, i);
    ox = g.cx, oy = g.cy, oz = g.cz;
    dx = g.rx, dy = g.ry, dz = g.rz;
  } else {
    const int pix = pixel_begin + i;
    const int py = pix / cam.width, px = pix - py * cam.width;
    const float off = cam.legacy_coord ? 0.0f : 0.5f;
    const float x = (float)px + off, y = (float)py + off;
    // [x y 1] @ Kinv^T, the chain of make_ray
    const float xn = __builtin_fmaf(y, cam.kinv[1], x * cam.kinv[0]) + cam.kinv[2];
    const float yn = __builtin_fmaf(y, cam.kinv[4], x * cam.kinv[3]) + cam.kinv[5];
    ox = cam.c2w[3], oy = cam.c2w[7], oz = cam.c2w[11];
    float cx, cy, cz;  // direction in the camera's frame
    if (cam.model == MNERF_CAM_ORTHO) {
      ox = dot4h_chain(xn, yn, 0.0f, cam.c2w + 0);
      oy = dot4h_chain(xn, yn, 0.0f, cam.c2w + 4);
      oz = dot4h_chain(xn, yn, 0.0f, cam.c2w + 8);
      cx = 0.0f, cy = 0.0f, cz = 1.0f;
    } else if (cam.model == MNERF_CAM_FISHEYE) {
      const float theta = sqrtf(xn * xn + yn * yn);
      const float s = cam_sin(theta, 0);
      const float inv = theta > 0.0f ? 1.0f / theta : 0.0f;  // theta = 0: the optical axis
      cx = s * (xn * inv), cy = s * (yn * inv), cz = cam_sin(theta, 1);
    } else {  // MNERF_CAM_SPHERE
      const float wn = cam.legacy_coord ? (float)max(cam.width - 1, 1) : (float)cam.width;
      const float hn = cam.legacy_coord ? (float)max(cam.height - 1, 1) : (float)cam.height;
      const float lon = __builtin_fmaf(x / wn, cam.lon_lat[1] - cam.lon_lat[0], cam.lon_lat[0]);
      const float lat = __builtin_fmaf(y / hn, cam.lon_lat[3] - cam.lon_lat[2], cam.lon_lat[2]);
      const float cl = cam_sin(lat, 1);
      cx = cl * cam_sin(lon, 0), cy = cam_sin(lat, 0), cz = cl * cam_sin(lon, 1);
    }
    dx = dot3_chain(cx, cy, cz, cam.c2w + 0);
    dy = dot3_chain(cx, cy, cz, cam.c2w + 4);
    dz = dot3_chain(cx, cy, cz, cam.c2w + 8);
    if (cam.model == MNERF_CAM_ORTHO) {  // c2w's z axis, normalised
      const float n = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
      dx = dx / n, dy = dy / n, dz = dz / n;
    }
  }
  float4* row = reinterpret_cast<float4*>(ray_od) + (size_t)i * 2;
  row[0] = make_float4(ox, oy, oz, 0.0f);
  row[1] = make_float4(dx, dy, dz, 0.0f);
}

extern "C" int mnerf_camera_rays(const void* camera, int32_t pixel_begin, int32_t n_pixels, float* ray_od, void* stream) {
  const mnerf_camera* cam = static_cast<const mnerf_camera*>(camera);
  MNERF_REQUIRE(cam, MNERF_E_NULL, "mnerf_camera_rays: camera is NULL");
  MNERF_REQUIRE(cam->model >= MNERF_CAM_PINHOLE && cam->model <= MNERF_CAM_ORTHO, MNERF_E_RANGE,
                "mnerf_camera_rays: model=%d is none of MNERF_CAM_*", cam->model);
  MNERF_REQUIRE(cam->height >= 1 && cam->width >= 1 && (long long)cam->height * cam->width < (1ll << 31), MNERF_E_RANGE,
                "mnerf_camera_rays: grid %dx%d", cam->height, cam->width);
  MNERF_REQUIRE(pixel_begin >= 0 && n_pixels >= 0 && (long long)pixel_begin + n_pixels <= (long long)cam->height * cam->width,
                MNERF_E_RANGE, "mnerf_camera_rays: pixels [%d, %d + %d) outside the %dx%d grid", pixel_begin, pixel_begin, n_pixels,
                cam->height, cam->width);
  if (n_pixels == 0) return MNERF_OK;
  MNERF_REQUIRE(ray_od, MNERF_E_NULL, "mnerf_camera_rays: ray_od is NULL");
  MNERF_REQUIRE(mnerf_aligned16(ray_od), MNERF_E_ALIGN, "mnerf_camera_rays: ray_od not 16B aligned");
  hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)(((long long)n_pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *cam,
                     pixel_begin, n_pixels, ray_od);
  return mnerf_check_launch("mnerf_camera_rays");
}

// ------------------------------------------------------------------------------------------------ per-sample geometry of a bundle
// One thread per sample, grid-stride (ray_samples_kernel of geometry.hip with the ray read from the bundle): sample_depth,
// ray_point and project give x_ndc / depth_s; dir is the ray's unit direction in view0's frame (the guard and the rotation of the
// decoder's own geometry, decoder.hip stage 10), the same for the S samples of a ray; ray_len = |d| is written by sample 0.
__global__ __launch_bounds__(256) void free_ray_samples_kernel(mnerf_rays R, mnerf_view V, const float* __restrict__ ray_od,
                                                               float* __restrict__ x_ndc, float* __restrict__ dir,
                                                               float* __restrict__ depth_s, float* __restrict__ ray_len) {
  const long long total = (long long)R.n_rays * R.n_samples;
  const float wm1 = (float)(R.width - 1), hm1 = (float)(R.height - 1);  // the SOURCE view's size
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ray = (int)(i / R.n_samples);
    const int j = (int)(i - (long long)ray * R.n_samples);
    const RayGeom g = ray_from_bundle(ray_od, ray);
    const float d = sample_depth(R, ray, j);
    if (depth_s) depth_s[i] = d;
    if (x_ndc) {
      float px, py, pz, u, v, z;
      ray_point(g, d, px, py, pz);
      project(V, px, py, pz, wm1, hm1, u, v, z);
      x_ndc[i * 3 + 0] = u;
      x_ndc[i * 3 + 1] = v;
      x_ndc[i * 3 + 2] = z;
    }
    const float len = sqrtf(g.rx * g.rx + g.ry * g.ry + g.rz * g.rz);
    if (ray_len && j == 0) ray_len[ray] = len;
    if (dir) {
      const float rn = fmaxf(len, 1e-12f);
      const float ux = g.rx / rn, uy = g.ry / rn, uz = g.rz / rn;
      dir[i * 3 + 0] = ux * V.extr[0] + uy * V.extr[1] + uz * V.extr[2];
      dir[i * 3 + 1] = ux * V.extr[4] + uy * V.extr[5] + uz * V.extr[6];
      dir[i * 3 + 2] = ux * V.extr[8] + uy * V.extr[9] + uz * V.extr[10];
    }
  }
}

extern "C" int mnerf_ray_samples_rays(const mnerf_rays* rays_in, const float* ray_od, const mnerf_view* view0, float* x_ndc,
                                      float* dir, float* depth_s, float* ray_len, void* stream) {
  mnerf_rays canon;
  if (const int rc = mnerf_free_rays_canonical(rays_in, ray_od, &canon, "mnerf_ray_samples_rays")) return rc;
  MNERF_REQUIRE((!x_ndc && !dir) || view0, MNERF_E_NULL, "mnerf_ray_samples_rays: view0 required for the x_ndc / dir outputs");
  MNERF_REQUIRE(!x_ndc || (canon.height >= 2 && canon.width >= 2), MNERF_E_RANGE, "mnerf_ray_samples_rays: image %dx%d",
                canon.height, canon.width);
  if (canon.n_rays == 0) return MNERF_OK;
  mnerf_view v = {};
  if (view0) v = *view0;
  const long long total = (long long)canon.n_rays * canon.n_samples;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(free_ray_samples_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, canon, v, ray_od, x_ndc,
                     dir, depth_s, ray_len);
  return mnerf_check_launch("mnerf_ray_samples_rays");
}
#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------ render chunk over a bundle
// workspace areas in floats (include/mnerf.h): cond | x_ndc | dir | depth_s | rgb_s | sigma | ray_len, each rounded up to 16 bytes
struct FreeRaysWorkspace {
  int64_t cond, x_ndc, dir, depth_s, rgb_s, sigma, ray_len, total;  // offsets in floats
};
static FreeRaysWorkspace free_rays_workspace(int64_t n_rays, int64_t n_samples, int64_t cond_stride) {
  const int64_t n = n_rays * n_samples;
  const auto up4 = [](int64_t x) { return (x + 3) & ~(int64_t)3; };
  FreeRaysWorkspace w;
  w.cond = 0;
  w.x_ndc = w.cond + up4(n * cond_stride);
  w.dir = w.x_ndc + up4(n * 3);
  w.depth_s = w.dir + up4(n * 3);
  w.rgb_s = w.depth_s + up4(n);
  w.sigma = w.rgb_s + up4(n * 3);
  w.ray_len = w.sigma + up4(n);
  w.total = w.ray_len + up4(n_rays);
  return w;
}

extern "C" int64_t mnerf_render_rays_workspace_bytes(int32_t n_rays, int32_t n_samples, int32_t cond_stride) {
  if (n_rays < 0 || n_samples < 1 || cond_stride < 1) return -1;
  return free_rays_workspace(n_rays, n_samples, cond_stride).total * (int64_t)sizeof(float);
}

extern "C" int mnerf_render_rays(const mnerf_scene* scene, const mnerf_decoder* dec, const mnerf_rays* rays_in, const float* ray_od,
                                 void* workspace, float* rgb, float* depth, float* opacity, void* stream) {
  MNERF_REQUIRE(scene && dec && rays_in, MNERF_E_NULL, "mnerf_render_rays: NULL argument struct");
  mnerf_rays canon;
  int rc = mnerf_free_rays_canonical(rays_in, ray_od, &canon, "mnerf_render_rays");
  if (rc) return rc;
  MNERF_REQUIRE(dec->n_views == scene->n_views, MNERF_E_RANGE, "mnerf_render_rays: decoder packed for %d views, scene has %d",
                dec->n_views, scene->n_views);
  const int sumG = scene->n_group[0] + (scene->n_scales > 1 ? scene->n_group[1] : 0);
  MNERF_REQUIRE(dec->cond_dim == sumG + 4 * scene->n_views, MNERF_E_RANGE, "mnerf_render_rays: cond_dim=%d != sum(cos_n_group)+4V=%d",
                dec->cond_dim, sumG + 4 * scene->n_views);
  MNERF_REQUIRE(dec->cond_stride >= 1, MNERF_E_RANGE, "mnerf_render_rays: cond_stride=%d", dec->cond_stride);
  if (canon.n_rays == 0) return MNERF_OK;
  MNERF_REQUIRE(rgb && depth && opacity, MNERF_E_NULL, "mnerf_render_rays: NULL output buffer");
  MNERF_REQUIRE(workspace, MNERF_E_NULL, "mnerf_render_rays: workspace is NULL");
  MNERF_REQUIRE(mnerf_aligned16(workspace), MNERF_E_ALIGN, "mnerf_render_rays: workspace not 16B aligned");
  // what the decoder's own step would refuse after the first two steps have been enqueued, as far as it can be told from here
  MNERF_REQUIRE(dec->wstream && dec->small_, MNERF_E_NULL, "mnerf_render_rays: NULL decoder weights");
  MNERF_REQUIRE(mnerf_aligned16(dec->wstream), MNERF_E_ALIGN, "mnerf_render_rays: wstream not 16B aligned");
  MNERF_REQUIRE(canon.n_samples <= 256, MNERF_E_UNSUPPORTED, "mnerf_render_rays: sample_intvs=%d > 256", canon.n_samples);
  const int64_t ws_floats = mnerf_decoder_wstream_floats(dec->cond_dim, dec->cond_stride, dec->L_3D, dec->wstream_format);
  MNERF_REQUIRE(ws_floats > 0 && ws_floats == dec->wstream_floats, ws_floats > 0 ? MNERF_E_RANGE : MNERF_E_UNSUPPORTED,
                "mnerf_render_rays: wstream has %lld floats, the decoder's schedule for this shape and format expects %lld",
                (long long)dec->wstream_floats, (long long)ws_floats);
  const FreeRaysWorkspace w = free_rays_workspace(canon.n_rays, canon.n_samples, dec->cond_stride);
  float* ws = (float*)workspace;
  rc = mnerf_cost_volume_rays(scene, &canon, ray_od, dec->cond_stride, ws + w.cond, stream);
  if (rc) return rc;
  rc = mnerf_ray_samples_rays(&canon, ray_od, &scene->views[0], ws + w.x_ndc, ws + w.dir, ws + w.depth_s, ws + w.ray_len, stream);
  if (rc) return rc;
  rc = mnerf_decoder_samples(dec, canon.n_rays, canon.n_samples, canon.legacy_coord, ws + w.x_ndc, ws + w.dir, ws + w.cond,
                             ws + w.rgb_s, ws + w.sigma, stream);
  if (rc) return rc;
  return mnerf_composite(canon.n_rays, canon.n_samples, ws + w.rgb_s, ws + w.sigma, ws + w.depth_s, ws + w.ray_len,
                         dec->wo_render_interval, dec->setbg_opaque, rgb, depth, opacity, nullptr, stream);
}
