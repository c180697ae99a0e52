// Mesh texture (include/mnerf.h "MESH TEXTURE"): a per-triangle atlas for an indexed mesh, baked from the views it was fused from.
//
// The layout is a function of (T, block) alone - two right-triangle patches per square block - so nothing is counted, packed or
// copied.  Memory-bound kernels of one thread per texel (x fastest, consecutive threads on consecutive texels, one float4 each):
//   texture_uv_kernel          per triangle: six half-integer numerators, one division each
//   texture_accumulate_kernel  per owned texel: its surface point, then per view one projection, four depth taps, the same taps of
//                              the colour; a read-modify-write of the texel's float4.  The views are summed inside the thread, in
//                              ascending order: no atomics of any kind
//   texture_resolve_kernel     per texel: the weighted mean (or the best view's colour), the vertex-colour blend where no view saw
//                              the surface, zeros where no triangle owns the texel
// The cameras travel by value in the kernel arguments, as the integrator's do.
#include <math.h>

#include "common.hpp"

// every operation rounds on its own; the FMAs are the explicit ones
#pragma clang fp contract(off)

#include "fusion_common.hpp"  // FusionCam, proj(), the value of a texel, the bilinear taps

constexpr int TEX_MIN_BLOCK = 4, TEX_MAX_BLOCK = 64, TEX_MAX_SIDE = 16384, TEX_MAX_POWER = 8;

struct TexLayout {
  int block, nbx, nby;  // the atlas is nbx x nby blocks
  int width, height;    // in texels
  long long n_triangles;
};

// false: beyond the header's bounds (of T, of block, of the atlas sides)
static bool tex_layout(long long n_triangles, int block, TexLayout* out) {
  if (n_triangles < 0 || 3 * (double)n_triangles >= 2147483648.0 || block < TEX_MIN_BLOCK || block > TEX_MAX_BLOCK) return false;
  const long long nb = n_triangles / 2 + n_triangles % 2;
  long long nbx = (long long)sqrt((double)nb);
  while (nbx * nbx < nb) ++nbx;
  while (nbx > 0 && (nbx - 1) * (nbx - 1) >= nb) --nbx;
  const long long nby = nbx ? (nb + nbx - 1) / nbx : 0;
  if (nbx * block > TEX_MAX_SIDE || nby * block > TEX_MAX_SIDE) return false;
  out->block = block, out->nbx = (int)nbx, out->nby = (int)nby;
  out->width = (int)nbx * block, out->height = (int)nby * block;
  out->n_triangles = n_triangles;
  return true;
}

static inline bool tex_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }
static inline unsigned tex_blocks(long long n) { return (unsigned)((n + PC_BLOCK - 1) / PC_BLOCK); }

// ------------------------------------------------------------------------------------------------ the texel -> surface map
// texel `i` of the atlas -> its triangle (-1: no owner) and the local texel (li, lj) of the triangle's patch
__device__ __forceinline__ long long tex_owner(const TexLayout& L, long long i, int& li, int& lj) {
  const int y = (int)(i / L.width), x = (int)(i - (long long)y * L.width);
  const int bx = x / L.block, by = y / L.block;
  li = x - bx * L.block, lj = y - by * L.block;
  long long t = 2 * ((long long)by * L.nbx + bx);
  if (li + lj >= L.block) {  // the upper triangle: the point reflection of the lower
    ++t;
    li = L.block - 1 - li, lj = L.block - 1 - lj;
  }
  return t < L.n_triangles ? t : -1;
}

// the surface coordinates of a local texel: the two rows past the hypotenuse are clamped onto it
__device__ __forceinline__ void tex_bary(int block, int li, int lj, float& a, float& b) {
  const float span = (float)(block - 3);
  a = (float)li / span, b = (float)lj / span;
  const float s = a + b;
  if (s > 1.0f) a = a / s, b = b / s;
}

struct TexTriangle {
  float4 p0, p1, p2;  // x y z w
  int v0, v1, v2;
  float nx, ny, nz, len;  // (p1 - p0) x (p2 - p0) and its length
};

// false: an index outside [0, V), a non-finite position or no area - the triangle takes no colour and shows none
__device__ __forceinline__ bool tex_triangle(const float* __restrict__ vertices, const int* __restrict__ triangles, long long t,
                                             int n_vertices, TexTriangle& tri) {
  tri.v0 = triangles[3 * t], tri.v1 = triangles[3 * t + 1], tri.v2 = triangles[3 * t + 2];
  if ((unsigned)tri.v0 >= (unsigned)n_vertices || (unsigned)tri.v1 >= (unsigned)n_vertices || (unsigned)tri.v2 >= (unsigned)n_vertices)
    return false;
  const float4* rows = reinterpret_cast<const float4*>(vertices);
  tri.p0 = rows[(size_t)tri.v0 * 2], tri.p1 = rows[(size_t)tri.v1 * 2], tri.p2 = rows[(size_t)tri.v2 * 2];
  const float ux = tri.p1.x - tri.p0.x, uy = tri.p1.y - tri.p0.y, uz = tri.p1.z - tri.p0.z;
  const float vx = tri.p2.x - tri.p0.x, vy = tri.p2.y - tri.p0.y, vz = tri.p2.z - tri.p0.z;
  if (!(isfinite(ux) && isfinite(uy) && isfinite(uz) && isfinite(vx) && isfinite(vy) && isfinite(vz) && isfinite(tri.p0.x) &&
        isfinite(tri.p0.y) && isfinite(tri.p0.z)))
    return false;
  tri.nx = __builtin_fmaf(uy, vz, -(uz * vy)), tri.ny = __builtin_fmaf(uz, vx, -(ux * vz)), tri.nz = __builtin_fmaf(ux, vy, -(uy * vx));
  tri.len = sqrtf(__builtin_fmaf(tri.nz, tri.nz, __builtin_fmaf(tri.ny, tri.ny, tri.nx * tri.nx)));
  return tri.len > 0.0f;
}

// q0 + a (q1 - q0) + b (q2 - q0): two FMAs
__device__ __forceinline__ float tex_blend(float a, float b, float q0, float q1, float q2) {
  return __builtin_fmaf(b, q2 - q0, __builtin_fmaf(a, q1 - q0, q0));
}

// ------------------------------------------------------------------------------------------------ uv
__global__ __launch_bounds__(PC_BLOCK) void texture_uv_kernel(TexLayout L, float* __restrict__ uv) {
  const long long t = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (t >= L.n_triangles) return;
  const long long p = t / 2;
  const float x0 = (float)((int)(p % L.nbx) * L.block), y0 = (float)((int)(p / L.nbx) * L.block);
  const float fb = (float)L.block, w = (float)L.width, h = (float)L.height;
  float cx[3], cy[3];
  if (t % 2 == 0) {
    cx[0] = 0.5f, cy[0] = 0.5f, cx[1] = fb - 2.5f, cy[1] = 0.5f, cx[2] = 0.5f, cy[2] = fb - 2.5f;
  } else {
    cx[0] = fb - 0.5f, cy[0] = fb - 0.5f, cx[1] = 2.5f, cy[1] = fb - 0.5f, cx[2] = fb - 0.5f, cy[2] = 2.5f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // (half-integers below 2^15: the sums are exact)
    uv[t * 6 + 2 * k] = (x0 + cx[k]) / w;
    uv[t * 6 + 2 * k + 1] = (y0 + cy[k]) / h;
  }
}

extern "C" int mnerf_mesh_texture_atlas(int64_t n_triangles, int32_t block, int32_t* size) {
  TexLayout L;
  MNERF_REQUIRE(tex_layout(n_triangles, block, &L), MNERF_E_RANGE,
                "mnerf_mesh_texture_atlas: %lld triangles in blocks of %d (block 4..64, 3 T < 2^31, sides <= 16384)",
                (long long)n_triangles, block);
  MNERF_REQUIRE(size, MNERF_E_NULL, "mnerf_mesh_texture_atlas: size is NULL");
  size[0] = L.width, size[1] = L.height;
  return MNERF_OK;
}

extern "C" int mnerf_mesh_texture_uv(int64_t n_triangles, int32_t block, float* uv, void* stream) {
  TexLayout L;
  MNERF_REQUIRE(tex_layout(n_triangles, block, &L), MNERF_E_RANGE,
                "mnerf_mesh_texture_uv: %lld triangles in blocks of %d (block 4..64, 3 T < 2^31, sides <= 16384)", (long long)n_triangles,
                block);
  if (n_triangles == 0) return MNERF_OK;
  MNERF_REQUIRE(uv, MNERF_E_NULL, "mnerf_mesh_texture_uv: uv is NULL");
  MNERF_REQUIRE(tex_aligned4(uv), MNERF_E_ALIGN, "mnerf_mesh_texture_uv: uv not 4B aligned");
  hipLaunchKernelGGL(texture_uv_kernel, dim3(tex_blocks(n_triangles)), dim3(PC_BLOCK), 0, (hipStream_t)stream, L, uv);
  return mnerf_check_launch("mnerf_mesh_texture_uv");
}

// ------------------------------------------------------------------------------------------------ accumulate
__global__ __launch_bounds__(PC_BLOCK) void texture_accumulate_kernel(
    TexLayout L, FusionCams cams, int n_views, const float* __restrict__ vertices, const int* __restrict__ triangles, int n_vertices,
    int height, int width, int legacy_coord, const float* __restrict__ depth, const float* __restrict__ opacity,
    const int* __restrict__ n_consistent, int min_consistent, const float* __restrict__ rgb, float min_opacity, float vis_rel_tol,
    int power, int best, float* __restrict__ accum) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= (long long)L.width * L.height) return;
  int li, lj;
  const long long t = tex_owner(L, i, li, lj);
  if (t < 0) return;
  TexTriangle tri;
  if (!tex_triangle(vertices, triangles, t, n_vertices, tri)) return;
  float a, b;
  tex_bary(L.block, li, lj, a, b);
  const float px = tex_blend(a, b, tri.p0.x, tri.p1.x, tri.p2.x);
  const float py = tex_blend(a, b, tri.p0.y, tri.p1.y, tri.p2.y);
  const float pz = tex_blend(a, b, tri.p0.z, tri.p1.z, tri.p2.z);
  const float off = legacy_coord ? 0.0f : 0.5f;
  const long long n = (long long)height * width;
  float4 acc = reinterpret_cast<const float4*>(accum)[i];
  for (int k = 0; k < n_views; ++k) {  // (wave-uniform: the cameras are read through scalar loads)
    const FusionCam& K = cams.cam[k];
    const float ex = K.c2w[3] - px, ey = K.c2w[7] - py, ez = K.c2w[11] - pz;
    const float elen = sqrtf(__builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)));
    const float cosv = __builtin_fmaf(tri.nz, ez, __builtin_fmaf(tri.ny, ey, tri.nx * ex)) / (tri.len * elen);
    if (!(cosv > 0.0f)) continue;  // the view looks at the back (or the quotient is a NaN)
    float u, v, zc;
    fusion_project(K, px, py, pz, u, v, zc);
    if (!(zc > 0.0f) || !fusion_in_frame(u, v, off, height, width)) continue;
    const FusionTaps taps = fusion_taps(u, v, off, height, width);
    const size_t base = (size_t)k * n;
    float d;
    if (!fusion_bilinear_value(depth, opacity, n_consistent, min_consistent, base, width, taps, min_opacity, K.v.near_, K.v.far_, d))
      continue;
    if (!(fabsf(d - zc) <= vis_rel_tol * zc)) continue;  // the view sees another surface in front of P
    const float* c00 = rgb + 3 * (base + (size_t)taps.y0 * width + taps.x0);
    const float* c10 = rgb + 3 * (base + (size_t)taps.y0 * width + taps.x1);
    const float* c01 = rgb + 3 * (base + (size_t)taps.y1 * width + taps.x0);
    const float* c11 = rgb + 3 * (base + (size_t)taps.y1 * width + taps.x1);
    const float r = fusion_bilinear(taps, c00[0], c10[0], c01[0], c11[0]);
    const float g = fusion_bilinear(taps, c00[1], c10[1], c01[1], c11[1]);
    const float bl = fusion_bilinear(taps, c00[2], c10[2], c01[2], c11[2]);
    float weight = 1.0f;
    for (int q = 0; q < power; ++q) weight = weight * cosv;
    if (best) {
      if (weight > acc.w) acc = make_float4(r, g, bl, weight);
    } else {
      acc.x = __builtin_fmaf(weight, r, acc.x);
      acc.y = __builtin_fmaf(weight, g, acc.y);
      acc.z = __builtin_fmaf(weight, bl, acc.z);
      acc.w = acc.w + weight;
    }
  }
  reinterpret_cast<float4*>(accum)[i] = acc;
}

// the checks the two mesh-taking entry points share; the layout comes back in *L
#define TEX_REQUIRE_MESH(who, V, T, block, L)                                                                                  \
  MNERF_REQUIRE((V) >= 0 && (V) < (1ll << 31), MNERF_E_RANGE, who ": %lld vertices", (long long)(V));                           \
  MNERF_REQUIRE(tex_layout((T), (block), (L)), MNERF_E_RANGE,                                                                 \
                who ": %lld triangles in blocks of %d (block 4..64, 3 T < 2^31, sides <= 16384)", (long long)(T), (block))

extern "C" int mnerf_mesh_texture_accumulate(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles,
                                             int32_t block, const mnerf_view* views, int32_t n_views, int32_t height, int32_t width,
                                             int32_t legacy_coord, const float* depth, const float* opacity, const int32_t* n_consistent,
                                             int32_t min_consistent, const float* rgb, float min_opacity, float vis_rel_tol,
                                             int32_t power, int32_t best, float* accum, void* stream) {
  TexLayout L;
  TEX_REQUIRE_MESH("mnerf_mesh_texture_accumulate", n_vertices, n_triangles, block, &L);
  MNERF_REQUIRE(n_views >= 1 && n_views <= MNERF_MAX_VIEWS, MNERF_E_RANGE, "mnerf_mesh_texture_accumulate: n_views=%d outside 1..%d",
                n_views, MNERF_MAX_VIEWS);
  MNERF_REQUIRE(height >= 1 && width >= 1 && (long long)height * width < (1ll << 31), MNERF_E_RANGE,
                "mnerf_mesh_texture_accumulate: maps %dx%d", height, width);
  MNERF_REQUIRE(!opacity || std::isfinite(min_opacity), MNERF_E_RANGE, "mnerf_mesh_texture_accumulate: min_opacity=%g",
                (double)min_opacity);
  MNERF_REQUIRE(std::isfinite(vis_rel_tol) && vis_rel_tol > 0.0f, MNERF_E_RANGE,
                "mnerf_mesh_texture_accumulate: vis_rel_tol=%g must be finite and positive", (double)vis_rel_tol);
  MNERF_REQUIRE(power >= 0 && power <= TEX_MAX_POWER, MNERF_E_RANGE, "mnerf_mesh_texture_accumulate: power=%d outside 0..%d", power,
                TEX_MAX_POWER);
  if (n_triangles == 0) return MNERF_OK;
  MNERF_REQUIRE((vertices || n_vertices == 0) && triangles && views, MNERF_E_NULL,
                "mnerf_mesh_texture_accumulate: NULL vertices / triangles / views");
  MNERF_REQUIRE(depth && rgb && accum, MNERF_E_NULL, "mnerf_mesh_texture_accumulate: NULL depth / rgb / accum");
  MNERF_REQUIRE(mnerf_aligned16(vertices) && mnerf_aligned16(accum), MNERF_E_ALIGN,
                "mnerf_mesh_texture_accumulate: vertices / accum not 16B aligned");
  MNERF_REQUIRE(tex_aligned4(triangles) && tex_aligned4(depth) && tex_aligned4(opacity) && tex_aligned4(n_consistent) && tex_aligned4(rgb),
                MNERF_E_ALIGN, "mnerf_mesh_texture_accumulate: triangles / depth / opacity / n_consistent / rgb not 4B aligned");
  FusionCams cams = {};
  for (int k = 0; k < n_views; ++k)
    MNERF_REQUIRE(fusion_cam(views[k], &cams.cam[k]), MNERF_E_RANGE, "mnerf_mesh_texture_accumulate: view %d has a singular intr or extr",
                  k);
  hipLaunchKernelGGL(texture_accumulate_kernel, dim3(tex_blocks((long long)L.width * L.height)), dim3(PC_BLOCK), 0, (hipStream_t)stream, L,
                     cams, n_views, vertices, triangles, (int)n_vertices, height, width, legacy_coord ? 1 : 0, depth, opacity, n_consistent,
                     min_consistent, rgb, min_opacity, vis_rel_tol, power, best ? 1 : 0, accum);
  return mnerf_check_launch("mnerf_mesh_texture_accumulate");
}

// ------------------------------------------------------------------------------------------------ resolve
// (accum and atlas may be one buffer: a thread reads its own texel before it writes it - hence no __restrict__ on the two)
__global__ __launch_bounds__(PC_BLOCK) void texture_resolve_kernel(TexLayout L, const float* __restrict__ vertices,
                                                                   const int* __restrict__ triangles, int n_vertices, int best,
                                                                   const float* accum, float* atlas) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= (long long)L.width * L.height) return;
  int li, lj;
  const long long t = tex_owner(L, i, li, lj);
  float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  TexTriangle tri;
  if (t >= 0 && tex_triangle(vertices, triangles, t, n_vertices, tri)) {
    const float4 acc = reinterpret_cast<const float4*>(accum)[i];
    if (acc.w > 0.0f) {
      out = best ? make_float4(acc.x, acc.y, acc.z, 1.0f) : make_float4(acc.x / acc.w, acc.y / acc.w, acc.z / acc.w, 1.0f);
    } else {  // no view saw the surface here: what the untextured mesh shows
      float a, b;
      tex_bary(L.block, li, lj, a, b);
      const float4* rows = reinterpret_cast<const float4*>(vertices);
      const float4 c0 = rows[(size_t)tri.v0 * 2 + 1], c1 = rows[(size_t)tri.v1 * 2 + 1], c2 = rows[(size_t)tri.v2 * 2 + 1];
      out = make_float4(tex_blend(a, b, c0.x, c1.x, c2.x), tex_blend(a, b, c0.y, c1.y, c2.y), tex_blend(a, b, c0.z, c1.z, c2.z), 0.0f);
    }
  }
  reinterpret_cast<float4*>(atlas)[i] = out;
}

extern "C" int mnerf_mesh_texture_resolve(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles,
                                          int32_t block, int32_t best, const float* accum, float* atlas, void* stream) {
  TexLayout L;
  TEX_REQUIRE_MESH("mnerf_mesh_texture_resolve", n_vertices, n_triangles, block, &L);
  if (n_triangles == 0) return MNERF_OK;
  MNERF_REQUIRE((vertices || n_vertices == 0) && triangles && accum && atlas, MNERF_E_NULL,
                "mnerf_mesh_texture_resolve: NULL vertices / triangles / accum / atlas");
  MNERF_REQUIRE(mnerf_aligned16(vertices) && mnerf_aligned16(accum) && mnerf_aligned16(atlas), MNERF_E_ALIGN,
                "mnerf_mesh_texture_resolve: vertices / accum / atlas not 16B aligned");
  MNERF_REQUIRE(tex_aligned4(triangles), MNERF_E_ALIGN, "mnerf_mesh_texture_resolve: triangles not 4B aligned");
  hipLaunchKernelGGL(texture_resolve_kernel, dim3(tex_blocks((long long)L.width * L.height)), dim3(PC_BLOCK), 0, (hipStream_t)stream, L,
                     vertices, triangles, (int)n_vertices, best ? 1 : 0, accum, atlas);
  return mnerf_check_launch("mnerf_mesh_texture_resolve");
}
#pragma clang fp contract(fast)
