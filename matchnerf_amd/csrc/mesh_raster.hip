// Mesh raster (include/mnerf.h "MESH RASTER"): the indexed mesh seen from one pinhole camera - a visibility buffer and its shading.
//
//   raster_clear_kernel    per pixel: the key becomes all ones
//   raster_kernel          one wave64 per triangle, four triangles per workgroup: the wave projects the three vertices, walks the
//                          8 x 8-pixel blocks of the clamped bounding box with lane = pixel, and issues one 64-bit unsigned atomicMin
//                          of (bits(z) << 32) | triangle per covered pixel.  An integer minimum over a set does not depend on the
//                          order of arrival: the winner is the same on every run.  No floating-point atomic, no scan, no expansion
//   raster_resolve_kernel  per pixel: the winner unpacked, its coverage quantities recomputed by the code that rasterized it
//   shade_kernel           per pixel: vertex colours or the atlas of MESH TEXTURE, and the face normal
// The camera travels by value in the kernel arguments, as the texture's do.
#include <math.h>

#include "common.hpp"

// every operation rounds on its own; the FMAs are the explicit ones
#pragma clang fp contract(off)

#include "fusion_common.hpp"  // FusionCam, proj(), the bilinear taps

constexpr int RASTER_TRIANGLES = PC_BLOCK / 64;  // per workgroup
constexpr int RASTER_MIN_BLOCK = 4, RASTER_MAX_BLOCK = 64, RASTER_MAX_SIDE = 16384;
constexpr unsigned long long RASTER_EMPTY = ~0ull;

static inline bool raster_aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
static inline unsigned raster_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// ------------------------------------------------------------------------------------------------ coverage
struct RasterTriangle {
  int v[3];
  float u[3], w[3], z[3];  // pixel coordinates (u across, w down) and camera-z of the three vertices
  float sign;              // of the orientation: +1 or -1
};

// the value of the edge a -> b at the pixel centre (px, py), from the edge's FIRST endpoint in (u, then v) order; `gx`, `gy`: the
// edge function's gradient before the orientation's sign (signs only)
__device__ __forceinline__ float raster_edge(float au, float av, float bu, float bv, float px, float py, float& gx, float& gy) {
  const bool swap = bu < au || (bu == au && bv < av);
  const float fu = swap ? bu : au, fv = swap ? bv : av, su = swap ? au : bu, sv = swap ? av : bv;
  const float dx = su - fu, dy = sv - fv;
  float e = __builtin_fmaf(dx, py - fv, -(dy * (px - fu)));
  if ((px == fu && py == fv) || (px == su && py == sv)) e = 0.0f;  // (the fma leaves the product's rounding error at the second)
  gx = swap ? dy : -dy, gy = swap ? -dx : dx;
  return swap ? -e : e;
}

// false: the triangle is dropped (an index outside [0, V), a position or projection that is not finite, a camera-z not > 0, no area)
__device__ __forceinline__ bool raster_triangle(const FusionCam& K, const float* __restrict__ vertices, const int* __restrict__ triangles,
                                                long long t, int n_vertices, RasterTriangle& tri) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    tri.v[k] = triangles[3 * t + k];
    ok &= (unsigned)tri.v[k] < (unsigned)n_vertices;
  }
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float4 p = reinterpret_cast<const float4*>(vertices)[(size_t)tri.v[k] * 2];
    fusion_project(K, p.x, p.y, p.z, tri.u[k], tri.w[k], tri.z[k]);
    ok &= isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(tri.u[k]) && isfinite(tri.w[k]) && isfinite(tri.z[k]) &&
          tri.z[k] > 0.0f;
  }
  if (!ok) return false;
  float gx, gy;
  const float area = raster_edge(tri.u[1], tri.w[1], tri.u[2], tri.w[2], tri.u[0], tri.w[0], gx, gy);
  if (!(area != 0.0f)) return false;
  tri.sign = area > 0.0f ? 1.0f : -1.0f;
  return true;
}

// covered: every oriented edge value > 0, or == 0 on an edge the triangle owns (its interior on the +x side; +y for a horizontal
// edge).  E[k] belongs to vertex k: the edge (k + 1) -> (k + 2).
__device__ __forceinline__ bool raster_covers(const RasterTriangle& tri, float px, float py, float E[3]) {
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    float gx, gy;
    const float e = raster_edge(tri.u[a], tri.w[a], tri.u[b], tri.w[b], px, py, gx, gy);
    E[k] = tri.sign * e;
    gx = tri.sign * gx, gy = tri.sign * gy;
    const bool owns = gx > 0.0f || (gx == 0.0f && gy > 0.0f);
    inside &= E[k] > 0.0f || (E[k] == 0.0f && owns);
  }
  return inside;
}

// perspective-correct depth and weights from the edge values; false: the sum of the edge values is not > 0
__device__ __forceinline__ bool raster_depth(const RasterTriangle& tri, const float E[3], float& z, float& b1, float& b2) {
  const float sum = (E[0] + E[1]) + E[2];
  if (!(sum > 0.0f)) return false;
  const float q0 = (E[0] / sum) / tri.z[0], q1 = (E[1] / sum) / tri.z[1], q2 = (E[2] / sum) / tri.z[2];
  const float w = (q0 + q1) + q2;
  z = 1.0f / w;
  b1 = q1 / w, b2 = q2 / w;
  return true;
}

// ------------------------------------------------------------------------------------------------ clear, raster, resolve
__global__ __launch_bounds__(PC_BLOCK) void raster_clear_kernel(long long n, unsigned long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i < n) keys[i] = RASTER_EMPTY;
}

__global__ __launch_bounds__(PC_BLOCK) void raster_kernel(FusionCam K, const float* __restrict__ vertices, const int* __restrict__ triangles,
                                                          int n_vertices, long long n_triangles, int height, int width, int legacy_coord,
                                                          unsigned long long* __restrict__ keys) {
  const long long t = (long long)blockIdx.x * RASTER_TRIANGLES + (threadIdx.x >> 6);
  if (t >= n_triangles) return;
  RasterTriangle tri;
  if (!raster_triangle(K, vertices, triangles, t, n_vertices, tri)) return;  // (wave-uniform)
  const float off = legacy_coord ? 0.0f : 0.5f;
  // the pixels whose centres can lie in the bounding box, one more on every side, clamped to the frame - in floats first: the
  // conversions below see values inside the frame only
  const float ulo = fminf(fminf(tri.u[0], tri.u[1]), tri.u[2]), uhi = fmaxf(fmaxf(tri.u[0], tri.u[1]), tri.u[2]);
  const float wlo = fminf(fminf(tri.w[0], tri.w[1]), tri.w[2]), whi = fmaxf(fmaxf(tri.w[0], tri.w[1]), tri.w[2]);
  const float fx0 = fmaxf(floorf(ulo - off) - 1.0f, 0.0f), fx1 = fminf(ceilf(uhi - off) + 1.0f, (float)(width - 1));
  const float fy0 = fmaxf(floorf(wlo - off) - 1.0f, 0.0f), fy1 = fminf(ceilf(whi - off) + 1.0f, (float)(height - 1));
  if (!(fx0 <= fx1 && fy0 <= fy1)) return;
  const int x0 = (int)fx0 & ~7, x1 = (int)fx1, y0 = (int)fy0 & ~7, y1 = (int)fy1;
  const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
  for (int by = y0; by <= y1; by += 8) {
    for (int bx = x0; bx <= x1; bx += 8) {
      const int x = bx + lx, y = by + ly;
      if (x >= width || y >= height) continue;
      float E[3], z, b1, b2;
      if (!raster_covers(tri, (float)x + off, (float)y + off, E)) continue;
      if (!raster_depth(tri, E, z, b1, b2)) continue;
      if (!(z > 0.0f && z >= K.v.near_ && z <= K.v.far_)) continue;  // (a NaN fails)
      const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(unsigned)t;
      atomicMin(keys + ((size_t)y * width + x), key);
    }
  }
}

__global__ __launch_bounds__(PC_BLOCK) void raster_resolve_kernel(FusionCam K, const float* __restrict__ vertices,
                                                                  const int* __restrict__ triangles, int n_vertices, long long n_triangles,
                                                                  int height, int width, int legacy_coord,
                                                                  const unsigned long long* __restrict__ keys, int* __restrict__ face,
                                                                  float* __restrict__ depth, float* __restrict__ bary) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= (long long)height * width) return;
  int f = -1;
  float z = 0.0f, b1 = 0.0f, b2 = 0.0f;
  const unsigned long long key = keys[i];
  const long long t = (long long)(key & 0xffffffffull);
  if (key != RASTER_EMPTY && t < n_triangles) {
    const int y = (int)(i / width), x = (int)(i - (long long)y * width);
    const float off = legacy_coord ? 0.0f : 0.5f;
    RasterTriangle tri;
    float E[3], zz, c1, c2;
    if (raster_triangle(K, vertices, triangles, t, n_vertices, tri) && raster_covers(tri, (float)x + off, (float)y + off, E) &&
        raster_depth(tri, E, zz, c1, c2))
      f = (int)t, z = zz, b1 = c1, b2 = c2;
  }
  face[i] = f;
  depth[i] = z;
  bary[2 * i] = b1, bary[2 * i + 1] = b2;
}

extern "C" int64_t mnerf_mesh_raster_workspace_bytes(int32_t height, int32_t width) {
  if (height < 1 || width < 1 || (long long)height * width >= (1ll << 31)) return -1;
  return 8ll * height * width;
}

// the bounds of the mesh that both entry points share
#define RASTER_REQUIRE_MESH(who, V, T)                                                                  \
  MNERF_REQUIRE((V) >= 0 && (V) < (1ll << 31), MNERF_E_RANGE, who ": %lld vertices", (long long)(V)); \
  MNERF_REQUIRE((T) >= 0 && 3 * (double)(T) < 2147483648.0, MNERF_E_RANGE, who ": %lld triangles (3 T < 2^31)", (long long)(T))

extern "C" int mnerf_mesh_raster(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles,
                                 const mnerf_view* view, int32_t height, int32_t width, int32_t legacy_coord, int32_t* face, float* depth,
                                 float* bary, void* workspace, int64_t workspace_bytes, void* stream) {
  RASTER_REQUIRE_MESH("mnerf_mesh_raster", n_vertices, n_triangles);
  const int64_t need = mnerf_mesh_raster_workspace_bytes(height, width);
  MNERF_REQUIRE(need >= 0, MNERF_E_RANGE, "mnerf_mesh_raster: a frame of %dx%d", height, width);
  MNERF_REQUIRE(workspace_bytes >= need, MNERF_E_RANGE, "mnerf_mesh_raster: a workspace of %lld bytes, the frame needs %lld",
                (long long)workspace_bytes, (long long)need);
  FusionCam cam = {};
  MNERF_REQUIRE(!view || fusion_cam(*view, &cam), MNERF_E_RANGE, "mnerf_mesh_raster: the view has a singular intr or extr");
  MNERF_REQUIRE(view && face && depth && bary && workspace, MNERF_E_NULL, "mnerf_mesh_raster: NULL view / face / depth / bary / workspace");
  MNERF_REQUIRE(n_triangles == 0 || ((vertices || n_vertices == 0) && triangles), MNERF_E_NULL,
                "mnerf_mesh_raster: NULL vertices / triangles");
  MNERF_REQUIRE(mnerf_aligned16(vertices) && raster_aligned(workspace, 8), MNERF_E_ALIGN,
                "mnerf_mesh_raster: vertices not 16B or workspace not 8B aligned");
  MNERF_REQUIRE(raster_aligned(triangles, 4) && raster_aligned(face, 4) && raster_aligned(depth, 4) && raster_aligned(bary, 4), MNERF_E_ALIGN,
                "mnerf_mesh_raster: triangles / face / depth / bary not 4B aligned");
  const long long n = (long long)height * width;
  const int legacy = legacy_coord ? 1 : 0;
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(raster_clear_kernel, dim3(raster_blocks(n, PC_BLOCK)), dim3(PC_BLOCK), 0, st, n, keys);
  if (n_triangles > 0)
    hipLaunchKernelGGL(raster_kernel, dim3(raster_blocks(n_triangles, RASTER_TRIANGLES)), dim3(PC_BLOCK), 0, st, cam, vertices, triangles,
                       (int)n_vertices, (long long)n_triangles, height, width, legacy, keys);
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(raster_blocks(n, PC_BLOCK)), dim3(PC_BLOCK), 0, st, cam, vertices, triangles, (int)n_vertices,
                     (long long)n_triangles, height, width, legacy, keys, face, depth, bary);
  return mnerf_check_launch("mnerf_mesh_raster");
}

// ------------------------------------------------------------------------------------------------ shade
struct RasterAtlas {
  int block, nbx, width, height;  // block == 0: no atlas
};

// the value of the atlas at tap (x, y) for the triangle whose block starts at (ox, oy): a tap the triangle does not own is read at
// the innermost tap (ix, iy) instead
__device__ __forceinline__ float4 raster_tap(const RasterAtlas& A, const float* __restrict__ atlas, int ox, int oy, bool upper, int x, int y,
                                             int ix, int iy) {
  const int li = x - ox, lj = y - oy;
  const bool in_block = li >= 0 && li < A.block && lj >= 0 && lj < A.block;
  const bool owned = in_block && (upper ? li + lj >= A.block : li + lj <= A.block - 1);
  if (!owned) x = ix, y = iy;
  return reinterpret_cast<const float4*>(atlas)[(size_t)y * A.width + x];
}

__global__ __launch_bounds__(PC_BLOCK) void shade_kernel(FusionCam K, RasterAtlas A, const float* __restrict__ vertices,
                                                         const int* __restrict__ triangles, int n_vertices, long long n_triangles,
                                                         const int* __restrict__ face, const float* __restrict__ bary, long long n,
                                                         const float* __restrict__ atlas, float* __restrict__ rgba,
                                                         float* __restrict__ normal) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n) return;
  float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nrm = out;
  const long long t = face[i];
  int v0 = -1, v1 = -1, v2 = -1;
  if (t >= 0 && t < n_triangles) v0 = triangles[3 * t], v1 = triangles[3 * t + 1], v2 = triangles[3 * t + 2];
  if ((unsigned)v0 < (unsigned)n_vertices && (unsigned)v1 < (unsigned)n_vertices && (unsigned)v2 < (unsigned)n_vertices) {
    const float b1 = bary[2 * i], b2 = bary[2 * i + 1];
    const float4* rows = reinterpret_cast<const float4*>(vertices);
    if (A.block == 0) {
      const float4 c0 = rows[(size_t)v0 * 2 + 1], c1 = rows[(size_t)v1 * 2 + 1], c2 = rows[(size_t)v2 * 2 + 1];
      out = make_float4(__builtin_fmaf(b2, c2.x - c0.x, __builtin_fmaf(b1, c1.x - c0.x, c0.x)),
                        __builtin_fmaf(b2, c2.y - c0.y, __builtin_fmaf(b1, c1.y - c0.y, c0.y)),
                        __builtin_fmaf(b2, c2.z - c0.z, __builtin_fmaf(b1, c1.z - c0.z, c0.z)), 1.0f);
    } else {
      const long long p = t / 2;
      const bool upper = t % 2 != 0;
      const int ox = (int)(p % A.nbx) * A.block, oy = (int)(p / A.nbx) * A.block;
      const float x0 = (float)ox, y0 = (float)oy, fb = (float)A.block;
      float cx[3], cy[3];  // the numerators of mnerf_mesh_texture_uv
      if (!upper) {
        cx[0] = x0 + 0.5f, cy[0] = y0 + 0.5f, cx[1] = x0 + (fb - 2.5f), cy[1] = y0 + 0.5f, cx[2] = x0 + 0.5f, cy[2] = y0 + (fb - 2.5f);
      } else {
        cx[0] = x0 + (fb - 0.5f), cy[0] = y0 + (fb - 0.5f), cx[1] = x0 + 2.5f, cy[1] = y0 + (fb - 0.5f), cx[2] = x0 + (fb - 0.5f),
        cy[2] = y0 + 2.5f;
      }
      const float tu = __builtin_fmaf(b2, cx[2] - cx[0], __builtin_fmaf(b1, cx[1] - cx[0], cx[0]));
      const float tv = __builtin_fmaf(b2, cy[2] - cy[0], __builtin_fmaf(b1, cy[1] - cy[0], cy[0]));
      FusionTaps taps = fusion_taps(tu, tv, 0.5f, A.height, A.width);
      if (taps.ax == 0.0f) taps.x1 = taps.x0;  // a tap of weight zero is not read
      if (taps.ay == 0.0f) taps.y1 = taps.y0;
      const int ix = upper ? taps.x1 : taps.x0, iy = upper ? taps.y1 : taps.y0;
      const float4 t00 = raster_tap(A, atlas, ox, oy, upper, taps.x0, taps.y0, ix, iy);
      const float4 t10 = raster_tap(A, atlas, ox, oy, upper, taps.x1, taps.y0, ix, iy);
      const float4 t01 = raster_tap(A, atlas, ox, oy, upper, taps.x0, taps.y1, ix, iy);
      const float4 t11 = raster_tap(A, atlas, ox, oy, upper, taps.x1, taps.y1, ix, iy);
      out = make_float4(fusion_bilinear(taps, t00.x, t10.x, t01.x, t11.x), fusion_bilinear(taps, t00.y, t10.y, t01.y, t11.y),
                        fusion_bilinear(taps, t00.z, t10.z, t01.z, t11.z), 1.0f);
    }
    if (normal) {
      const float4 p0 = rows[(size_t)v0 * 2], p1 = rows[(size_t)v1 * 2], p2 = rows[(size_t)v2 * 2];
      const float ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
      const float vx = p2.x - p0.x, vy = p2.y - p0.y, vz = p2.z - p0.z;
      const float nx = __builtin_fmaf(uy, vz, -(uz * vy)), ny = __builtin_fmaf(uz, vx, -(ux * vz)), nz = __builtin_fmaf(ux, vy, -(uy * vx));
      const float len = sqrtf(__builtin_fmaf(nz, nz, __builtin_fmaf(ny, ny, nx * nx)));
      if (len > 0.0f && isfinite(len)) {
        const float ex = K.c2w[3] - p0.x, ey = K.c2w[7] - p0.y, ez = K.c2w[11] - p0.z;
        const float towards = __builtin_fmaf(nz, ez, __builtin_fmaf(ny, ey, nx * ex));
        const float s = towards < 0.0f ? -1.0f : 1.0f;
        nrm = make_float4(s * (nx / len), s * (ny / len), s * (nz / len), 0.0f);
      }
    }
  }
  reinterpret_cast<float4*>(rgba)[i] = out;
  if (normal) reinterpret_cast<float4*>(normal)[i] = nrm;
}

extern "C" int mnerf_mesh_shade(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, const int32_t* face,
                                const float* bary, int32_t height, int32_t width, const float* atlas, int32_t atlas_height,
                                int32_t atlas_width, int32_t block, const mnerf_view* view, float* rgba, float* normal, void* stream) {
  RASTER_REQUIRE_MESH("mnerf_mesh_shade", n_vertices, n_triangles);
  MNERF_REQUIRE(height >= 1 && width >= 1 && (long long)height * width < (1ll << 31), MNERF_E_RANGE, "mnerf_mesh_shade: a frame of %dx%d",
                height, width);
  RasterAtlas A = {};
  if (atlas) {
    MNERF_REQUIRE(block >= RASTER_MIN_BLOCK && block <= RASTER_MAX_BLOCK, MNERF_E_RANGE, "mnerf_mesh_shade: block=%d outside 4..64", block);
    const long long nb = n_triangles / 2 + n_triangles % 2;  // the layout of mnerf_mesh_texture_atlas
    long long nbx = (long long)sqrt((double)nb);
    while (nbx * nbx < nb) ++nbx;
    while (nbx > 0 && (nbx - 1) * (nbx - 1) >= nb) --nbx;
    const long long nby = nbx ? (nb + nbx - 1) / nbx : 0;
    MNERF_REQUIRE(nbx * block <= RASTER_MAX_SIDE && nby * block <= RASTER_MAX_SIDE && atlas_width == nbx * block && atlas_height == nby * block,
                  MNERF_E_RANGE, "mnerf_mesh_shade: an atlas of %dx%d, %lld triangles in blocks of %d have %lldx%lld (sides <= 16384)",
                  atlas_width, atlas_height, (long long)n_triangles, block, nbx * block, nby * block);
    A.block = block, A.nbx = (int)nbx, A.width = atlas_width, A.height = atlas_height;
  }
  FusionCam cam = {};
  MNERF_REQUIRE(!view || fusion_cam(*view, &cam), MNERF_E_RANGE, "mnerf_mesh_shade: the view has a singular intr or extr");
  MNERF_REQUIRE(view && face && bary && rgba, MNERF_E_NULL, "mnerf_mesh_shade: NULL view / face / bary / rgba");
  MNERF_REQUIRE(n_triangles == 0 || ((vertices || n_vertices == 0) && triangles), MNERF_E_NULL,
                "mnerf_mesh_shade: NULL vertices / triangles");
  MNERF_REQUIRE(mnerf_aligned16(vertices) && mnerf_aligned16(atlas) && mnerf_aligned16(rgba) && mnerf_aligned16(normal), MNERF_E_ALIGN,
                "mnerf_mesh_shade: vertices / atlas / rgba / normal not 16B aligned");
  MNERF_REQUIRE(raster_aligned(triangles, 4) && raster_aligned(face, 4) && raster_aligned(bary, 4), MNERF_E_ALIGN,
                "mnerf_mesh_shade: triangles / face / bary not 4B aligned");
  if (n_triangles == 0) A.block = 0;  // (an empty atlas: every pixel is 0 0 0 0 anyway)
  const long long n = (long long)height * width;
  hipLaunchKernelGGL(shade_kernel, dim3(raster_blocks(n, PC_BLOCK)), dim3(PC_BLOCK), 0, (hipStream_t)stream, cam, A, vertices, triangles,
                     (int)n_vertices, (long long)n_triangles, face, bary, n, atlas, rgba, normal);
  return mnerf_check_launch("mnerf_mesh_shade");
}
#pragma clang fp contract(fast)
