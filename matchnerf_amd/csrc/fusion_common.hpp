// What the geometry-export kernels share (fusion.hip: consistency, point cloud; mesh.hip: TSDF volume, mesher; mesh_finish.hip:
// finishing, decimation; mesh_texture.hip: the atlas): the camera with its host-inverted matrices, the fp32 projection chain, the
// value of a depth texel, the bilinear taps, the integer workgroup scans of the stable compactions with the two-level scan over them (scan.hip), and the carving of a workspace.
// Include after common.hpp, under `#pragma clang fp contract(off)`: every operation rounds on its own and the FMAs are the explicit
// ones of the helpers.
#pragma once
#include <math.h>

#include "common.hpp"

struct FusionCam {
  mnerf_view v;     // world -> camera, intrinsics, valid depth range
  float kinv[9];    // intr^-1, inverted in double on the host
  float c2w[12];    // [R^-1 | -R^-1 t], inverted in double on the host
};
struct FusionCams {
  FusionCam cam[MNERF_MAX_VIEWS];
};

// pixel-centre coordinates (x, y) at camera-z `z` -> world
__device__ __forceinline__ void fusion_lift(const FusionCam& c, float x, float y, float z, float& wx, float& wy, float& wz) {
  // cam = [x y 1] @ Kinv^T, the chain of make_ray; then every component times the depth
  const float c0 = (__builtin_fmaf(y, c.kinv[1], x * c.kinv[0]) + c.kinv[2]) * z;
  const float c1 = (__builtin_fmaf(y, c.kinv[4], x * c.kinv[3]) + c.kinv[5]) * z;
  const float c2 = (__builtin_fmaf(y, c.kinv[7], x * c.kinv[6]) + c.kinv[8]) * z;
  wx = dot4h_chain(c0, c1, c2, c.c2w + 0);
  wy = dot4h_chain(c0, c1, c2, c.c2w + 4);
  wz = dot4h_chain(c0, c1, c2, c.c2w + 8);
}

// world -> pixel coordinates and camera-z (project() of common.hpp without the normalisations)
__device__ __forceinline__ void fusion_project(const FusionCam& c, float wx, float wy, float wz, float& u, float& v, float& z) {
  const float c0 = dot4h_chain(wx, wy, wz, c.v.extr + 0);
  const float c1 = dot4h_chain(wx, wy, wz, c.v.extr + 4);
  const float c2 = dot4h_chain(wx, wy, wz, c.v.extr + 8);
  const float q0 = dot3_chain(c0, c1, c2, c.v.intr + 0);
  const float q1 = dot3_chain(c0, c1, c2, c.v.intr + 3);
  const float q2 = dot3_chain(c0, c1, c2, c.v.intr + 6);
  u = q0 / q2;
  v = q1 / q2;
  z = q2;
}

// the value of pixel `i` of view `k`'s map: normalised by the opacity where one is given; false = invalid
__device__ __forceinline__ bool fusion_value(const float* __restrict__ depth, const float* __restrict__ opacity, size_t i,
                                             float min_opacity, float near_, float far_, float& z) {
  z = depth[i];
  if (opacity) {
    const float o = opacity[i];
    if (!(o >= min_opacity)) return false;  // a NaN opacity is invalid
    z = z / o;
  }
  return isfinite(z) && z >= near_ && z <= far_;
}

// the bilinear taps of a map at pixel coordinates (u, v) inside the rectangle of its pixel centres (include/mnerf.h
// "mnerf_depth_consistency"): the texels (x0|x1, y0|y1) and the weights ax, ay of x1 and y1
struct FusionTaps {
  int x0, y0, x1, y1;
  float ax, ay;
};
__device__ __forceinline__ bool fusion_in_frame(float u, float v, float off, int height, int width) {
  return u >= off && u <= (float)(width - 1) + off && v >= off && v <= (float)(height - 1) + off;
}
__device__ __forceinline__ FusionTaps fusion_taps(float u, float v, float off, int height, int width) {
  FusionTaps t;
  const float fx = u - off, fy = v - off;
  t.x0 = max(min((int)floorf(fx), width - 2), 0), t.y0 = max(min((int)floorf(fy), height - 2), 0);
  t.x1 = min(t.x0 + 1, width - 1), t.y1 = min(t.y0 + 1, height - 1);
  t.ax = fx - (float)t.x0, t.ay = fy - (float)t.y0;
  return t;
}
// top + ay (bot - top) with top = v00 + ax (v10 - v00), bot = v01 + ax (v11 - v01), each a + t b one FMA
__device__ __forceinline__ float fusion_bilinear(const FusionTaps& t, float v00, float v10, float v01, float v11) {
  const float top = __builtin_fmaf(t.ax, v10 - v00, v00);
  const float bot = __builtin_fmaf(t.ax, v11 - v01, v01);
  return __builtin_fmaf(t.ay, bot - top, top);
}
// the bilinear value of a view's map (`base` = its first pixel) at the taps; false unless all four texels are VALID, whatever their
// weights, and - with n_consistent - confirmed by min_consistent views
__device__ __forceinline__ bool fusion_bilinear_value(const float* __restrict__ depth, const float* __restrict__ opacity,
                                                      const int* __restrict__ n_consistent, int min_consistent, size_t base,
                                                      int width, const FusionTaps& t, float min_opacity, float near_, float far_,
                                                      float& z) {
  const size_t i00 = base + (size_t)t.y0 * width + t.x0, i10 = base + (size_t)t.y0 * width + t.x1;
  const size_t i01 = base + (size_t)t.y1 * width + t.x0, i11 = base + (size_t)t.y1 * width + t.x1;
  float z00, z10, z01, z11;
  bool ok = fusion_value(depth, opacity, i00, min_opacity, near_, far_, z00);
  ok &= fusion_value(depth, opacity, i10, min_opacity, near_, far_, z10);
  ok &= fusion_value(depth, opacity, i01, min_opacity, near_, far_, z01);
  ok &= fusion_value(depth, opacity, i11, min_opacity, near_, far_, z11);
  if (n_consistent)
    ok &= n_consistent[i00] >= min_consistent && n_consistent[i10] >= min_consistent && n_consistent[i01] >= min_consistent &&
          n_consistent[i11] >= min_consistent;
  z = fusion_bilinear(t, z00, z10, z01, z11);
  return ok;
}

// ------------------------------------------------------------------------------------------------ host: inverse cameras
static bool invert3(const double* m, double* inv) {  // row-major 3x3 by the adjugate
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  if (!(fabs(det) > 0.0) || !std::isfinite(det)) return false;
  const double r = 1.0 / det;
  inv[0] = c00 * r, inv[1] = (m[2] * m[7] - m[1] * m[8]) * r, inv[2] = (m[1] * m[5] - m[2] * m[4]) * r;
  inv[3] = c01 * r, inv[4] = (m[0] * m[8] - m[2] * m[6]) * r, inv[5] = (m[2] * m[3] - m[0] * m[5]) * r;
  inv[6] = c02 * r, inv[7] = (m[1] * m[6] - m[0] * m[7]) * r, inv[8] = (m[0] * m[4] - m[1] * m[3]) * r;
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(inv[k])) return false;
  return true;
}

static bool fusion_cam(const mnerf_view& v, FusionCam* out) {
  double k[9], ki[9], r[9], ri[9];
  for (int i = 0; i < 9; ++i) k[i] = v.intr[i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[i * 3 + j] = v.extr[i * 4 + j];
  if (!invert3(k, ki) || !invert3(r, ri)) return false;
  out->v = v;
  for (int i = 0; i < 9; ++i) out->kinv[i] = (float)ki[i];
  for (int i = 0; i < 3; ++i) {
    double t = 0.0;
    for (int j = 0; j < 3; ++j) {
      out->c2w[i * 4 + j] = (float)ri[i * 3 + j];
      t -= ri[i * 3 + j] * (double)v.extr[j * 4 + 3];
    }
    out->c2w[i * 4 + 3] = (float)t;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------ workgroup scans
constexpr int PC_BLOCK = 256;    // elements per workgroup of the count / scatter kernels
constexpr int PC_TILE = 1024;    // counts per workgroup of the scan: 256 threads x 4

// selected pixels before this lane in the workgroup (ballots + the waves' totals through LDS); `total` = the workgroup's count
__device__ __forceinline__ int block_prefix(bool flag, int& total) {
  __shared__ int wave_count[PC_BLOCK / 64];
  const unsigned long long mask = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int before = __popcll(mask & ((1ull << lane) - 1ull));
  if (lane == 0) wave_count[wave] = __popcll(mask);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < PC_BLOCK / 64; ++w) {
    const int c = wave_count[w];
    base += w < wave ? c : 0;
    total += c;
  }
  return base + before;
}

// exclusive scan of up to PC_TILE values held four per thread; returns the thread's first prefix, `total` = the sum of all
__device__ __forceinline__ int tile_scan(const int v[4], int& total) {
  __shared__ int wave_sum[PC_BLOCK / 64];
  const int mine = v[0] + v[1] + v[2] + v[3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  __syncthreads();  // (a caller's loop: the previous round's reads of wave_sum are over)
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < PC_BLOCK / 64; ++w) {
    const int c = wave_sum[w];
    base += w < wave ? c : 0;
    total += c;
  }
  return base + incl - mine;
}

// ------------------------------------------------------------------------------------------------ the two-level scan (scan.hip)
// A count kernel leaves one int32 per workgroup of PC_BLOCK elements in `counts`.  scan_enqueue turns every count into the exclusive
// prefix inside its tile of PC_TILE workgroups, `tiles` into the tiles' exclusive prefixes, and writes the grand total - two
// launches, or the second alone over an empty range (the total, 0, is written all the same; nothing with an empty grid is launched).
// A scatter kernel of the same grid then places its workgroup's elements from scan_row.  Every prefix is below 2^31 (the entry
// points bound their sizes so), hence the int32 tables.
struct ScanScratch {  // int32 [blocks] | int32 [n_tiles], one after the other in a workspace
  int *counts, *tiles;
  long long blocks, n_tiles;
};
static inline long long scan_blocks(long long n) { return n / PC_BLOCK + (n % PC_BLOCK != 0); }  // (no n + 255: any int64 n >= 0)
static inline long long scan_tiles(long long n) { return (scan_blocks(n) + PC_TILE - 1) / PC_TILE; }

void scan_enqueue(const ScanScratch& s, long long* total, hipStream_t st);
// the same over values[n], one per thread, that no count kernel has summed: the workgroups' sums first (three launches)
void scan_values_enqueue(const int* values, int n, const ScanScratch& s, long long* total, hipStream_t st);
// The offsets of a CSR table from its rows' lengths: offsets[0 .. n) hold the counts and become their exclusive prefixes,
// offsets[n] = the total (also in *total), cursor[0 .. n) = a copy for a fill that advances it; n >= 1.  scan_values_enqueue plus
// one launch.
void csr_offsets_enqueue(int* offsets, int n, const ScanScratch& s, long long* total, int* cursor, hipStream_t st);

// the output row of a workgroup's element that has `before` selected elements of the same workgroup in front of it
__device__ __forceinline__ long long scan_row(const int* __restrict__ counts, const int* __restrict__ tiles, int before) {
  return (long long)tiles[blockIdx.x / PC_TILE] + counts[blockIdx.x] + before;
}

// ------------------------------------------------------------------------------------------------ host: carving a workspace
// A layout is a list of requests: each returns its array at the running offset rounded up to the alignment.  With a null base only
// the offsets and the total mean anything - that is how the *_workspace_bytes functions size what the entry points carve.
struct Carve {
  char* base;
  size_t at = 0;
  explicit Carve(void* workspace) : base(static_cast<char*>(workspace)) {}
  size_t take(size_t bytes, size_t alignment) {
    const size_t offset = (at + alignment - 1) & ~(alignment - 1);
    at = offset + bytes;
    return offset;
  }
  template <typename T>
  T* array(size_t count, size_t alignment = alignof(T)) {
    return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + take(count * sizeof(T), alignment));
  }
  ScanScratch scan(long long n) {  // the scratch of one scan over n elements, a single request
    ScanScratch s;
    s.blocks = scan_blocks(n), s.n_tiles = scan_tiles(n);
    s.counts = array<int>((size_t)s.blocks), s.tiles = array<int>((size_t)s.n_tiles);
    return s;
  }
  long long bytes() const { return (long long)((at + 15) & ~(size_t)15); }  // the total: a multiple of 16
};
