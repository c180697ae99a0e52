// Geometry export (include/mnerf.h "GEOMETRY EXPORT"): cross-view consistency of rendered depth maps, the stable compaction of the
// surviving pixels into a coloured point cloud, and the colour map of the depth panels.
//
// All three are memory-bound kernels of one thread per pixel, consecutive threads on consecutive pixels:
//   depth_consistency_kernel   per pixel of the reference view and per partner: two projections, four taps, two more projections
//   point_count / the scan (scan.hip) / point_scatter   wave ballots + a two-level scan of the workgroups' counts: the rows
//                              come out in pixel order without an atomic cursor, so that two runs give the same bits
//   depth_colormap_kernel      one load, three byte stores
// The cameras travel by value in the kernel arguments (as mnerf_scene's views do): 16 x 44 floats.
#include <math.h>

#include "common.hpp"

// every operation rounds on its own; the FMAs are the explicit ones of the helpers (common.hpp)
#pragma clang fp contract(off)

#include "fusion_common.hpp"  // FusionCam, the projection chain, fusion_value, the scan and the workspace carve

__global__ __launch_bounds__(256) void depth_consistency_kernel(FusionCams cams, int n_views, int ref, int height, int width,
                                                                int legacy_coord, const float* __restrict__ depth,
                                                                const float* __restrict__ opacity, float px_tol, float rel_tol,
                                                                float min_opacity, float* __restrict__ fused_depth,
                                                                int* __restrict__ n_consistent) {
  const long long n = (long long)height * width;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int py = (int)(i / width), px = (int)(i - (long long)py * width);
  const float off = legacy_coord ? 0.0f : 0.5f;
  const float x = (float)px + off, y = (float)py + off;
  const FusionCam& R = cams.cam[ref];
  float z;
  if (!fusion_value(depth, opacity, (size_t)ref * n + i, min_opacity, R.v.near_, R.v.far_, z)) {
    n_consistent[i] = 0;
    fused_depth[i] = 0.0f;
    return;
  }
  float wx, wy, wz;
  fusion_lift(R, x, y, z, wx, wy, wz);
  int count = 0;
  float sum = z;
  for (int j = 0; j < n_views; ++j) {  // (wave-uniform: the cameras are read through scalar loads)
    if (j == ref) continue;
    const FusionCam& J = cams.cam[j];
    float u, v, zj;
    fusion_project(J, wx, wy, wz, u, v, zj);
    if (!(zj > 0.0f) || !fusion_in_frame(u, v, off, height, width)) continue;
    const FusionTaps t = fusion_taps(u, v, off, height, width);
    float dj;
    if (!fusion_bilinear_value(depth, opacity, nullptr, 0, (size_t)j * n, width, t, min_opacity, J.v.near_, J.v.far_, dj)) continue;
    float bx, by, bz, xr, yr, dr;
    fusion_lift(J, u, v, dj, bx, by, bz);
    fusion_project(R, bx, by, bz, xr, yr, dr);
    const float ex = xr - x, ey = yr - y;
    const float err = sqrtf(ex * ex + ey * ey);
    if (err < px_tol && fabsf(dr - z) < rel_tol * z) {
      ++count;
      sum = sum + dr;
    }
  }
  n_consistent[i] = count;
  fused_depth[i] = sum / (float)(1 + count);
}

extern "C" int mnerf_depth_consistency(const mnerf_view* views, int32_t n_views, int32_t ref, int32_t height, int32_t width,
                                       int32_t legacy_coord, const float* depth, const float* opacity, float px_tol, float rel_tol,
                                       float min_opacity, float* fused_depth, int32_t* n_consistent, void* stream) {
  MNERF_REQUIRE(n_views >= 2 && n_views <= MNERF_MAX_VIEWS, MNERF_E_RANGE, "mnerf_depth_consistency: n_views=%d outside 2..%d", n_views,
                MNERF_MAX_VIEWS);
  MNERF_REQUIRE(ref >= 0 && ref < n_views, MNERF_E_RANGE, "mnerf_depth_consistency: ref=%d outside the %d views", ref, n_views);
  MNERF_REQUIRE(height >= 1 && width >= 1 && (long long)height * width < (1ll << 31), MNERF_E_RANGE,
                "mnerf_depth_consistency: grid %dx%d", height, width);
  MNERF_REQUIRE(std::isfinite(px_tol) && px_tol > 0.0f && std::isfinite(rel_tol) && rel_tol > 0.0f, MNERF_E_RANGE,
                "mnerf_depth_consistency: px_tol=%g rel_tol=%g must be finite and positive", (double)px_tol, (double)rel_tol);
  MNERF_REQUIRE(!opacity || std::isfinite(min_opacity), MNERF_E_RANGE, "mnerf_depth_consistency: min_opacity=%g", (double)min_opacity);
  MNERF_REQUIRE(views, MNERF_E_NULL, "mnerf_depth_consistency: views is NULL");
  MNERF_REQUIRE(depth && fused_depth && n_consistent, MNERF_E_NULL, "mnerf_depth_consistency: NULL depth / fused_depth / n_consistent");
  FusionCams cams = {};
  for (int k = 0; k < n_views; ++k)
    MNERF_REQUIRE(fusion_cam(views[k], &cams.cam[k]), MNERF_E_RANGE, "mnerf_depth_consistency: view %d has a singular intr or extr", k);
  const long long n = (long long)height * width;
  hipLaunchKernelGGL(depth_consistency_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cams, n_views, ref,
                     height, width, legacy_coord ? 1 : 0, depth, opacity, px_tol, rel_tol, min_opacity, fused_depth, n_consistent);
  return mnerf_check_launch("mnerf_depth_consistency");
}

// ------------------------------------------------------------------------------------------------ point cloud
// Workspace: the scratch of one scan over the pixels.  Every prefix is below 2^31 (height x width is).

__device__ __forceinline__ bool point_selected(const float* __restrict__ depth, const int* __restrict__ n_consistent,
                                               int min_consistent, long long i, long long n) {
  if (i >= n) return false;
  if (n_consistent[i] < min_consistent) return false;
  const float d = depth[i];
  return isfinite(d) && d > 0.0f;
}

__global__ __launch_bounds__(PC_BLOCK) void point_count_kernel(const float* __restrict__ depth, const int* __restrict__ n_consistent,
                                                               int min_consistent, long long n, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int total;
  block_prefix(point_selected(depth, n_consistent, min_consistent, i, n), total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void point_scatter_kernel(FusionCam cam, int width, int legacy_coord,
                                                                 const float* __restrict__ depth, const float* __restrict__ rgb,
                                                                 const int* __restrict__ n_consistent, int min_consistent, long long n,
                                                                 const int* __restrict__ counts, const int* __restrict__ tiles,
                                                                 float* __restrict__ points, long long capacity) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const bool flag = point_selected(depth, n_consistent, min_consistent, i, n);
  int total;
  const int before = block_prefix(flag, total);
  if (!flag) return;
  const long long row = scan_row(counts, tiles, before);
  if (row >= capacity) return;
  const int py = (int)(i / width), px = (int)(i - (long long)py * width);
  const float off = legacy_coord ? 0.0f : 0.5f;
  const float d = depth[i];
  float wx, wy, wz;
  fusion_lift(cam, (float)px + off, (float)py + off, d, wx, wy, wz);
  float4* out = reinterpret_cast<float4*>(points) + (size_t)row * 2;
  out[0] = make_float4(wx, wy, wz, d);
  out[1] = make_float4(rgb[i * 3 + 0], rgb[i * 3 + 1], rgb[i * 3 + 2], (float)n_consistent[i]);
}

extern "C" int64_t mnerf_point_cloud_workspace_bytes(int64_t n_pixels) {
  if (n_pixels < 0) return -1;
  Carve sizes(nullptr);
  sizes.scan(n_pixels);
  return sizes.bytes();
}

extern "C" int mnerf_point_cloud(const mnerf_view* view, int32_t height, int32_t width, int32_t legacy_coord, const float* depth,
                                 const float* rgb, const int32_t* n_consistent, int32_t min_consistent, float* points,
                                 int64_t capacity, int64_t* count, void* workspace, void* stream) {
  MNERF_REQUIRE(height >= 0 && width >= 0 && (long long)height * width < (1ll << 31), MNERF_E_RANGE, "mnerf_point_cloud: grid %dx%d",
                height, width);
  MNERF_REQUIRE(capacity >= 0, MNERF_E_RANGE, "mnerf_point_cloud: capacity=%lld", (long long)capacity);
  const long long n = (long long)height * width;
  if (n == 0) return MNERF_OK;
  MNERF_REQUIRE(view, MNERF_E_NULL, "mnerf_point_cloud: view is NULL");
  MNERF_REQUIRE(depth && rgb && n_consistent && count && workspace, MNERF_E_NULL,
                "mnerf_point_cloud: NULL depth / rgb / n_consistent / count / workspace");
  MNERF_REQUIRE(capacity == 0 || points, MNERF_E_NULL, "mnerf_point_cloud: points is NULL");
  MNERF_REQUIRE(mnerf_aligned16(points), MNERF_E_ALIGN, "mnerf_point_cloud: points not 16B aligned");
  MNERF_REQUIRE((((uintptr_t)workspace) & 3u) == 0 && (((uintptr_t)count) & 7u) == 0, MNERF_E_ALIGN,
                "mnerf_point_cloud: workspace / count not aligned to 4 / 8 bytes");
  FusionCam cam;
  MNERF_REQUIRE(fusion_cam(*view, &cam), MNERF_E_RANGE, "mnerf_point_cloud: the view has a singular intr or extr");
  const ScanScratch s = Carve(workspace).scan(n);
  const dim3 blocks((unsigned)s.blocks), threads(PC_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(point_count_kernel, blocks, threads, 0, st, depth, n_consistent, min_consistent, n, s.counts);
  scan_enqueue(s, reinterpret_cast<long long*>(count), st);
  hipLaunchKernelGGL(point_scatter_kernel, blocks, threads, 0, st, cam, width, legacy_coord ? 1 : 0, depth, rgb, n_consistent,
                     min_consistent, n, s.counts, s.tiles, points, (long long)capacity);
  return mnerf_check_launch("mnerf_point_cloud");
}

// ------------------------------------------------------------------------------------------------ colour map
__device__ __forceinline__ unsigned char jet_channel(int index, int centre) {  // 255 clamp(1.5 - |4 s - c|) rounded half up, exactly
  return (unsigned char)min(max(383 - abs(4 * index - centre), 0), 255);
}

__global__ __launch_bounds__(256) void depth_colormap_kernel(const float* __restrict__ depth, long long n, float lo, float denom,
                                                             unsigned char* __restrict__ rgb) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float d = depth[i];
    if (d != d) d = 0.0f;
    const float t = 255.0f * ((d - lo) / denom);
    const int index = !(t > 0.0f) ? 0 : (t >= 255.0f ? 255 : (int)t);
    rgb[i * 3 + 0] = jet_channel(index, 765);
    rgb[i * 3 + 1] = jet_channel(index, 510);
    rgb[i * 3 + 2] = jet_channel(index, 255);
  }
}

extern "C" int mnerf_depth_colormap(const float* depth, int64_t n, float lo, float hi, uint8_t* rgb, void* stream) {
  MNERF_REQUIRE(n >= 0, MNERF_E_RANGE, "mnerf_depth_colormap: n=%lld", (long long)n);
  MNERF_REQUIRE(std::isfinite(lo) && std::isfinite(hi), MNERF_E_RANGE, "mnerf_depth_colormap: lo=%g hi=%g", (double)lo, (double)hi);
  if (n == 0) return MNERF_OK;
  MNERF_REQUIRE(depth && rgb, MNERF_E_NULL, "mnerf_depth_colormap: NULL depth / rgb");
  const float denom = (float)((double)hi - (double)lo + 1e-8);
  long long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(depth_colormap_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, depth, (long long)n, lo, denom, rgb);
  return mnerf_check_launch("mnerf_depth_colormap");
}
#pragma clang fp contract(fast)
