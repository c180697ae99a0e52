// Mesh export on a BRICK-SPARSE volume (include/mnerf.h "SPARSE TSDF VOLUME"): the volume of mesh.hip stored only where a surface can
// be.  A brick is 8 x 8 x 8 voxels; a table over the bricks of the virtual grid gives each allocated brick its slot.
//   tsdf_bricks_mark_kernel        one workgroup per brick of the virtual grid: the integrator's per-view step (tsdf_common.hpp, the
//                                  very function tsdf_integrate_kernel calls) per voxel; a voxel some view updates with t < 1 marks
//                                  the bricks of its 3 x 3 x 3 neighbourhood
//   bricks_count / the scan (scan.hip) / bricks_scatter   marks -> table and the list of the allocated bricks, ascending
//   tsdf_integrate_sparse_kernel   one workgroup per allocated brick: the dense update on the voxel's global index
//   smesh_*                        the nine launches of the dense mesher over the n_bricks x 512 allocated points; a neighbour is
//                                  found through the table
// No atomics anywhere: a mark is a plain store of 1, every row's place comes from the integer scans.
#include <math.h>

#include <algorithm>

#include "common.hpp"

// every operation rounds on its own; the FMAs are the explicit ones
#pragma clang fp contract(off)

#include "fusion_common.hpp"
#include "tsdf_common.hpp"

constexpr int BRICK = MNERF_TSDF_BRICK;               // voxels per side
constexpr int BRICK_POINTS = BRICK * BRICK * BRICK;   // 512
static_assert(BRICK == 8 && BRICK_POINTS % PC_BLOCK == 0, "the in-brick index is three 3-bit fields; a workgroup never straddles bricks");
constexpr long long SPARSE_MAX_BRICKS = MESH_MAX_POINTS / BRICK_POINTS;  // 349 525
constexpr long long MARK_LAUNCH_BRICKS = 1ll << 22;                      // bricks of the virtual grid per launch of the mark

struct BrickGrid {
  int bx, by, bz;
};
static inline int bricks_of(int n) { return n / BRICK + (n % BRICK != 0); }  // (no n + 7: any int32 n >= 0)
static BrickGrid brick_grid(int nx, int ny, int nz) { return {bricks_of(nx), bricks_of(ny), bricks_of(nz)}; }
static bool brick_grid_ok(const BrickGrid& b) { return (double)b.bx * (double)b.by * (double)b.bz < 2147483648.0; }

// the brick with the linear index `brick` -> the global index of its first voxel along every axis
__device__ __forceinline__ void brick_corner(int brick, BrickGrid b, int& x0, int& y0, int& z0) {
  x0 = (brick % b.bx) * BRICK, y0 = ((brick / b.bx) % b.by) * BRICK, z0 = (brick / (b.bx * b.by)) * BRICK;  // (bx by bz < 2^31)
}

// ------------------------------------------------------------------------------------------------ mark
__global__ __launch_bounds__(PC_BLOCK) void tsdf_bricks_mark_kernel(FusionCams cams, int n_views, TsdfMaps maps, TsdfGrid g, BrickGrid b,
                                                                    int first, unsigned char* __restrict__ marks) {
  __shared__ int wanted[27];  // [dz + 1][dy + 1][dx + 1]: a NEAR voxel of this brick has a neighbour in that brick
  if (threadIdx.x < 27) wanted[threadIdx.x] = 0;
  __syncthreads();
  int x0, y0, z0;
  brick_corner(first + (int)blockIdx.x, b, x0, y0, z0);
#pragma unroll
  for (int half = 0; half < BRICK_POINTS / PC_BLOCK; ++half) {
    const int local = half * PC_BLOCK + threadIdx.x;
    const int lx = local & 7, ly = local >> 3 & 7, lz = local >> 6;
    const int ix = x0 + lx, iy = y0 + ly, iz = z0 + lz;
    if (ix >= g.nx || iy >= g.ny || iz >= g.nz) continue;  // a partial brick
    const float px = voxel_centre(ix, g.voxel, g.ox), py = voxel_centre(iy, g.voxel, g.oy), pz = voxel_centre(iz, g.voxel, g.oz);
    bool near = false;
    for (int j = 0; j < n_views && !near; ++j) {
      size_t texel;
      float t;
      near = tsdf_view_step(cams.cam[j], j, maps, px, py, pz, texel, t) && t < 1.0f;
    }
    if (!near) continue;
    // the neighbours ix - 1 .. ix + 1 inside the grid: the brick below when lx == 0, the brick above when lx == 7
    const int xlo = (lx == 0 && ix > 0) ? -1 : 0, xhi = (lx == BRICK - 1 && ix + 1 < g.nx) ? 1 : 0;
    const int ylo = (ly == 0 && iy > 0) ? -1 : 0, yhi = (ly == BRICK - 1 && iy + 1 < g.ny) ? 1 : 0;
    const int zlo = (lz == 0 && iz > 0) ? -1 : 0, zhi = (lz == BRICK - 1 && iz + 1 < g.nz) ? 1 : 0;
    for (int dz = zlo; dz <= zhi; ++dz)
      for (int dy = ylo; dy <= yhi; ++dy)
        for (int dx = xlo; dx <= xhi; ++dx) wanted[((dz + 1) * 3 + dy + 1) * 3 + dx + 1] = 1;  // (racing stores of the same value)
  }
  __syncthreads();
  if (threadIdx.x < 27 && wanted[threadIdx.x]) {
    const int dx = (int)threadIdx.x % 3 - 1, dy = (int)threadIdx.x / 3 % 3 - 1, dz = (int)threadIdx.x / 9 - 1;
    const int cx = x0 / BRICK + dx, cy = y0 / BRICK + dy, cz = z0 / BRICK + dz;  // inside the brick grid by the tests above
    marks[((long long)cz * b.by + cy) * b.bx + cx] = 1;
  }
}

// the checks the mark and the sparse integrator share with mnerf_tsdf_integrate; fills the cameras
static int sparse_maps_ok(const char* who, const mnerf_view* views, int32_t n_views, int32_t height, int32_t width, const float* opacity,
                          float min_opacity, float trunc, float ox, float oy, float oz, float voxel, int32_t nx, int32_t ny, int32_t nz) {
  MNERF_REQUIRE(n_views >= 1 && n_views <= MNERF_MAX_VIEWS, MNERF_E_RANGE, "%s: n_views=%d outside 1..%d", who, n_views, MNERF_MAX_VIEWS);
  MNERF_REQUIRE(height >= 1 && width >= 1 && (long long)height * width < (1ll << 31), MNERF_E_RANGE, "%s: maps %dx%d", who, height, width);
  MNERF_REQUIRE(std::isfinite(trunc) && trunc > 0.0f, MNERF_E_RANGE, "%s: trunc=%g must be finite and positive", who, (double)trunc);
  MNERF_REQUIRE(!opacity || std::isfinite(min_opacity), MNERF_E_RANGE, "%s: min_opacity=%g", who, (double)min_opacity);
  MNERF_REQUIRE(grid_ok(ox, oy, oz, voxel, nx, ny, nz), MNERF_E_RANGE, "%s: grid %dx%dx%d of voxel %g at (%g, %g, %g)", who, nx, ny, nz,
                (double)voxel, (double)ox, (double)oy, (double)oz);
  MNERF_REQUIRE(brick_grid_ok(brick_grid(nx, ny, nz)), MNERF_E_RANGE, "%s: grid %dx%dx%d has 2^31 bricks or more", who, nx, ny, nz);
  return MNERF_OK;
}
static int sparse_cams(const char* who, const mnerf_view* views, int32_t n_views, FusionCams* cams) {
  for (int k = 0; k < n_views; ++k)
    MNERF_REQUIRE(fusion_cam(views[k], &cams->cam[k]), MNERF_E_RANGE, "%s: view %d has a singular intr or extr", who, k);
  return MNERF_OK;
}

extern "C" int mnerf_tsdf_bricks_mark(const mnerf_view* views, int32_t n_views, int32_t height, int32_t width, int32_t legacy_coord,
                                      const float* depth, const float* opacity, const int32_t* n_consistent, int32_t min_consistent,
                                      float min_opacity, float trunc, float origin_x, float origin_y, float origin_z, float voxel,
                                      int32_t nx, int32_t ny, int32_t nz, uint8_t* marks, void* stream) {
  const char* who = "mnerf_tsdf_bricks_mark";
  if (const int rc = sparse_maps_ok(who, views, n_views, height, width, opacity, min_opacity, trunc, origin_x, origin_y, origin_z, voxel,
                                    nx, ny, nz))
    return rc;
  const BrickGrid b = brick_grid(nx, ny, nz);
  const long long n_all = (long long)b.bx * b.by * b.bz;
  if (n_all == 0) return MNERF_OK;
  MNERF_REQUIRE(views, MNERF_E_NULL, "%s: views is NULL", who);
  MNERF_REQUIRE(depth && marks, MNERF_E_NULL, "%s: NULL depth / marks", who);
  FusionCams cams = {};
  if (const int rc = sparse_cams(who, views, n_views, &cams)) return rc;
  const TsdfMaps maps = {height, width, legacy_coord ? 1 : 0, depth, opacity, n_consistent, min_consistent, min_opacity, trunc};
  const TsdfGrid g = {origin_x, origin_y, origin_z, voxel, nx, ny, nz};
  for (long long first = 0; first < n_all; first += MARK_LAUNCH_BRICKS)  // (one launch up to 1024^3 voxels; a launch's threads stay below 2^32)
    hipLaunchKernelGGL(tsdf_bricks_mark_kernel, dim3((unsigned)std::min(n_all - first, MARK_LAUNCH_BRICKS)), dim3(PC_BLOCK), 0,
                       (hipStream_t)stream, cams, n_views, maps, g, b, (int)first, marks);
  return mnerf_check_launch(who);
}

// ------------------------------------------------------------------------------------------------ table
__global__ __launch_bounds__(PC_BLOCK) void bricks_count_kernel(const unsigned char* __restrict__ marks, int n, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int total;
  block_prefix(i < n && marks[i] != 0, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void bricks_scatter_kernel(const unsigned char* __restrict__ marks, int n,
                                                                  const int* __restrict__ counts, const int* __restrict__ tiles,
                                                                  int* __restrict__ table, int* __restrict__ bricks) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const bool marked = i < n && marks[i] != 0;
  int total;
  const int before = block_prefix(marked, total);
  if (i >= n) return;
  const int slot = (int)scan_row(counts, tiles, before);
  table[i] = marked ? slot : -1;
  if (marked) bricks[slot] = (int)i;
}

static bool brick_dims_ok(int32_t bx, int32_t by, int32_t bz) {
  return bx >= 0 && by >= 0 && bz >= 0 && (double)bx * (double)by * (double)bz < 2147483648.0;
}

extern "C" int64_t mnerf_tsdf_bricks_table_workspace_bytes(int32_t bx, int32_t by, int32_t bz) {
  if (!brick_dims_ok(bx, by, bz)) return -1;
  Carve c(nullptr);
  c.scan((long long)bx * by * bz);
  return c.bytes();
}

extern "C" int mnerf_tsdf_bricks_table(const uint8_t* marks, int32_t bx, int32_t by, int32_t bz, int32_t* table, int32_t* bricks,
                                       int64_t* count, void* workspace, void* stream) {
  const char* who = "mnerf_tsdf_bricks_table";
  MNERF_REQUIRE(brick_dims_ok(bx, by, bz), MNERF_E_RANGE, "%s: %dx%dx%d bricks: a size below 0, or 2^31 bricks or more", who, bx, by, bz);
  const long long n = (long long)bx * by * bz;
  MNERF_REQUIRE(count, MNERF_E_NULL, "%s: count is NULL", who);
  MNERF_REQUIRE(n == 0 || (marks && table && bricks && workspace), MNERF_E_NULL, "%s: NULL marks / table / bricks / workspace", who);
  MNERF_REQUIRE((((uintptr_t)table) & 3u) == 0 && (((uintptr_t)bricks) & 3u) == 0 && (((uintptr_t)workspace) & 3u) == 0 &&
                    (((uintptr_t)count) & 7u) == 0,
                MNERF_E_ALIGN, "%s: table / bricks / workspace / count not aligned to 4 / 4 / 4 / 8 bytes", who);
  Carve c(workspace);
  const ScanScratch s = c.scan(n);
  hipStream_t st = (hipStream_t)stream;
  if (s.blocks) hipLaunchKernelGGL(bricks_count_kernel, dim3((unsigned)s.blocks), dim3(PC_BLOCK), 0, st, marks, (int)n, s.counts);
  scan_enqueue(s, reinterpret_cast<long long*>(count), st);
  if (s.blocks)
    hipLaunchKernelGGL(bricks_scatter_kernel, dim3((unsigned)s.blocks), dim3(PC_BLOCK), 0, st, marks, (int)n, s.counts, s.tiles, table, bricks);
  return mnerf_check_launch(who);
}

// ------------------------------------------------------------------------------------------------ integration
__global__ __launch_bounds__(PC_BLOCK) void tsdf_integrate_sparse_kernel(FusionCams cams, int n_views, TsdfMaps maps,
                                                                         const float* __restrict__ rgb, TsdfGrid g, BrickGrid b,
                                                                         const int* __restrict__ bricks, float* __restrict__ sums,
                                                                         float* __restrict__ weight) {
  int x0, y0, z0;
  brick_corner(bricks[blockIdx.x], b, x0, y0, z0);
#pragma unroll
  for (int half = 0; half < BRICK_POINTS / PC_BLOCK; ++half) {
    const int local = half * PC_BLOCK + threadIdx.x;
    const int ix = x0 + (local & 7), iy = y0 + (local >> 3 & 7), iz = z0 + (local >> 6);
    if (ix >= g.nx || iy >= g.ny || iz >= g.nz) continue;  // a partial brick: never updated
    const size_t i = (size_t)blockIdx.x * BRICK_POINTS + local;
    const float px = voxel_centre(ix, g.voxel, g.ox), py = voxel_centre(iy, g.voxel, g.oy), pz = voxel_centre(iz, g.voxel, g.oz);
    float4 acc = reinterpret_cast<const float4*>(sums)[i];
    float wsum = weight[i];
    for (int j = 0; j < n_views; ++j) {
      size_t texel;
      float t;
      if (!tsdf_view_step(cams.cam[j], j, maps, px, py, pz, texel, t)) continue;
      acc.x = acc.x + t;
      acc.y = acc.y + rgb[texel * 3 + 0];
      acc.z = acc.z + rgb[texel * 3 + 1];
      acc.w = acc.w + rgb[texel * 3 + 2];
      wsum = wsum + 1.0f;
    }
    reinterpret_cast<float4*>(sums)[i] = acc;
    weight[i] = wsum;
  }
}

// n_bricks against the table's size and the int32 row bound of the mesher
static int sparse_bricks_ok(const char* who, int64_t n_bricks, const BrickGrid& b) {
  MNERF_REQUIRE(n_bricks >= 0 && n_bricks <= (long long)b.bx * b.by * b.bz, MNERF_E_RANGE, "%s: n_bricks=%lld outside 0..%lld, the table's size",
                who, (long long)n_bricks, (long long)b.bx * b.by * b.bz);
  MNERF_REQUIRE(n_bricks <= SPARSE_MAX_BRICKS, MNERF_E_RANGE, "%s: n_bricks=%lld above %lld (512 points each, 12 triangle rows per point below 2^31)",
                who, (long long)n_bricks, SPARSE_MAX_BRICKS);
  return MNERF_OK;
}

extern "C" int mnerf_tsdf_integrate_sparse(const mnerf_view* views, int32_t n_views, int32_t height, int32_t width, int32_t legacy_coord,
                                           const float* depth, const float* opacity, const int32_t* n_consistent, int32_t min_consistent,
                                           const float* rgb, float min_opacity, float trunc, float origin_x, float origin_y,
                                           float origin_z, float voxel, int32_t nx, int32_t ny, int32_t nz, const int32_t* bricks,
                                           int64_t n_bricks, float* sums, float* weight, void* stream) {
  const char* who = "mnerf_tsdf_integrate_sparse";
  if (const int rc = sparse_maps_ok(who, views, n_views, height, width, opacity, min_opacity, trunc, origin_x, origin_y, origin_z, voxel,
                                    nx, ny, nz))
    return rc;
  const BrickGrid b = brick_grid(nx, ny, nz);
  if (const int rc = sparse_bricks_ok(who, n_bricks, b)) return rc;
  if (n_bricks == 0) return MNERF_OK;
  MNERF_REQUIRE(views, MNERF_E_NULL, "%s: views is NULL", who);
  MNERF_REQUIRE(depth && rgb && bricks && sums && weight, MNERF_E_NULL, "%s: NULL depth / rgb / bricks / sums / weight", who);
  MNERF_REQUIRE(mnerf_aligned16(sums), MNERF_E_ALIGN, "%s: sums not 16B aligned", who);
  MNERF_REQUIRE((((uintptr_t)weight) & 3u) == 0 && (((uintptr_t)bricks) & 3u) == 0, MNERF_E_ALIGN, "%s: weight / bricks not 4B aligned", who);
  FusionCams cams = {};
  if (const int rc = sparse_cams(who, views, n_views, &cams)) return rc;
  const TsdfMaps maps = {height, width, legacy_coord ? 1 : 0, depth, opacity, n_consistent, min_consistent, min_opacity, trunc};
  const TsdfGrid g = {origin_x, origin_y, origin_z, voxel, nx, ny, nz};
  hipLaunchKernelGGL(tsdf_integrate_sparse_kernel, dim3((unsigned)n_bricks), dim3(PC_BLOCK), 0, (hipStream_t)stream, cams, n_views, maps,
                     rgb, g, b, bricks, sums, weight);
  return mnerf_check_launch(who);
}

// ------------------------------------------------------------------------------------------------ mesher
// An allocated point is p = slot x 512 + the in-brick index (k 8 + j) 8 + i; below 2^31 / 12 by the bound on n_bricks.
struct SparseLattice {
  const int* __restrict__ table;
  const int* __restrict__ bricks;
  int nx, ny, nz;
  BrickGrid b;
};
// where a thread's point lies
struct SparsePoint {
  int p, slot, ix, iy, iz;  // ix..: the global index; outside the grid in a partial brick
};
__device__ __forceinline__ SparsePoint sparse_point(const SparseLattice& s, long long p) {
  SparsePoint q;
  q.p = (int)p, q.slot = (int)(p / BRICK_POINTS);
  const int local = (int)(p % BRICK_POINTS);
  int x0, y0, z0;
  brick_corner(s.bricks[q.slot], s.b, x0, y0, z0);
  q.ix = x0 + (local & 7), q.iy = y0 + (local >> 3 & 7), q.iz = z0 + (local >> 6);
  return q;
}
__device__ __forceinline__ bool sparse_in_grid(const SparseLattice& s, int x, int y, int z) {
  return x >= 0 && y >= 0 && z >= 0 && x < s.nx && y < s.ny && z < s.nz;
}
// the point at q + (dx, dy, dz), each in -1..1: -1 outside the grid or in a brick without a slot
__device__ __forceinline__ int sparse_neighbour(const SparseLattice& s, const SparsePoint& q, int dx, int dy, int dz) {
  const int x = q.ix + dx, y = q.iy + dy, z = q.iz + dz;
  if (!sparse_in_grid(s, x, y, z)) return -1;
  int slot = q.slot;
  if (((x ^ q.ix) | (y ^ q.iy) | (z ^ q.iz)) >> 3)  // another brick
    slot = s.table[((z >> 3) * s.b.by + (y >> 3)) * s.b.bx + (x >> 3)];
  return slot < 0 ? -1 : slot * BRICK_POINTS + (((z & 7) * 8 + (y & 7)) * 8 + (x & 7));
}

__global__ __launch_bounds__(PC_BLOCK) void smesh_flags_kernel(const float* __restrict__ weight, const float* __restrict__ sums,
                                                               float min_weight, SparseLattice s, unsigned char* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;  // (the grid is exactly n_bricks x 512 / 256 workgroups)
  const SparsePoint q = sparse_point(s, i);
  unsigned char f = 0;
  if (sparse_in_grid(s, q.ix, q.iy, q.iz)) {
    const float w = weight[i];
    if (w >= min_weight) {
      f = MF_VALID;
      if (sums[i * 4] / w < 0.0f) f |= MF_INSIDE;
      bool all = true;
#pragma unroll
      for (int c = 1; c < 8; ++c) {
        const int j = sparse_neighbour(s, q, c & 1, c >> 1 & 1, c >> 2);
        all &= j >= 0 && weight[j >= 0 ? j : 0] >= min_weight;
      }
      if (all) f |= MF_CELL;
    }
  }
  flags[i] = f;
}

// live_edges of mesh.hip through the table: a valid cell's corners are all allocated, so every point read below exists
__device__ __forceinline__ int sparse_live_edges(const unsigned char* __restrict__ flags, const SparseLattice& s, const SparsePoint& q) {
  int cells = 0;  // bit f: the cell at q - f exists and is valid
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    const int j = sparse_neighbour(s, q, -(f & 1), -(f >> 1 & 1), -(f >> 2));
    if (j >= 0 && (flags[j] & MF_CELL)) cells |= 1 << f;
  }
  if (!cells) return 0;
  const int inside = flags[q.p] & MF_INSIDE;
  int mask = 0;
#pragma unroll
  for (int e = 1; e < 8; ++e) {
    int users = 0;
#pragma unroll
    for (int f = 0; f < 8; ++f)
      if (!(f & e)) users |= 1 << f;
    if (!(cells & users)) continue;  // (then q + e is a corner of a valid cell)
    const int j = sparse_neighbour(s, q, e & 1, e >> 1 & 1, e >> 2);
    if (j >= 0 && (flags[j] & MF_INSIDE) != inside) mask |= 1 << (e - 1);
  }
  return mask;
}

__global__ __launch_bounds__(PC_BLOCK) void smesh_vcount_kernel(const unsigned char* __restrict__ flags, SparseLattice s,
                                                                unsigned char* __restrict__ masks, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const int mask = sparse_live_edges(flags, s, sparse_point(s, i));
  masks[i] = (unsigned char)mask;
  const int v[4] = {(int)__popc(mask), 0, 0, 0};
  int total;
  tile_scan(v, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void smesh_vscatter_kernel(const float* __restrict__ sums, const float* __restrict__ weight,
                                                                  TsdfGrid g, SparseLattice s, const unsigned char* __restrict__ masks,
                                                                  const int* __restrict__ counts, const int* __restrict__ tiles,
                                                                  int* __restrict__ vbase, float* __restrict__ vertices,
                                                                  long long capacity) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const int mask = masks[i];
  const int v[4] = {(int)__popc(mask), 0, 0, 0};
  int total;
  const int before = tile_scan(v, total);
  long long row = scan_row(counts, tiles, before);
  vbase[i] = (int)row;
  if (!mask) return;
  const SparsePoint q = sparse_point(s, i);
  const float4 sa = reinterpret_cast<const float4*>(sums)[i];
  const float wa = weight[i];
  const float da = sa.x / wa, ra = sa.y / wa, ga = sa.z / wa, ba = sa.w / wa;
  const float ax = voxel_centre(q.ix, g.voxel, g.ox), ay = voxel_centre(q.iy, g.voxel, g.oy), az = voxel_centre(q.iz, g.voxel, g.oz);
#pragma unroll
  for (int e = 1; e < 8; ++e) {
    if (!(mask >> (e - 1) & 1)) continue;
    if (row >= capacity) return;
    const int ex = e & 1, ey = e >> 1 & 1, ez = e >> 2;
    const int j = sparse_neighbour(s, q, ex, ey, ez);  // (>= 0: a live edge's far end is a corner of a valid cell)
    const float4 sb = reinterpret_cast<const float4*>(sums)[j];
    const float wb = weight[j];
    const float db = sb.x / wb, rb = sb.y / wb, gb = sb.z / wb, bb = sb.w / wb;
    const float bx = voxel_centre(q.ix + ex, g.voxel, g.ox), by = voxel_centre(q.iy + ey, g.voxel, g.oy),
                bz = voxel_centre(q.iz + ez, g.voxel, g.oz);
    const float t = da / (da - db);
    float4* out = reinterpret_cast<float4*>(vertices) + (size_t)row * 2;
    out[0] = make_float4(__builtin_fmaf(t, bx - ax, ax), __builtin_fmaf(t, by - ay, ay), __builtin_fmaf(t, bz - az, az),
                         __builtin_fmaf(t, wb - wa, wa));
    out[1] = make_float4(__builtin_fmaf(t, rb - ra, ra), __builtin_fmaf(t, gb - ga, ga), __builtin_fmaf(t, bb - ba, ba), 0.0f);
    ++row;
  }
}

// the points of the 8 corners of the cell at q and the table rows of its six tets; returns the triangles the cell emits
__device__ __forceinline__ int sparse_cell_triangles(const unsigned char* __restrict__ flags, const SparseLattice& s, const SparsePoint& q,
                                                     int corner[8], int rows[6]) {
  int cell = -1;
  if (flags[q.p] & MF_CELL) {  // (then all 8 corners are allocated)
    cell = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      corner[c] = sparse_neighbour(s, q, c & 1, c >> 1 & 1, c >> 2);
      if (flags[corner[c]] & MF_INSIDE) cell |= 1 << c;
    }
  }
  return cell_rows(cell, rows);
}

__global__ __launch_bounds__(PC_BLOCK) void smesh_tcount_kernel(const unsigned char* __restrict__ flags, SparseLattice s,
                                                                int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int corner[8], rows[6];
  const int v[4] = {sparse_cell_triangles(flags, s, sparse_point(s, i), corner, rows), 0, 0, 0};
  int total;
  tile_scan(v, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void smesh_tscatter_kernel(const unsigned char* __restrict__ flags,
                                                                  const unsigned char* __restrict__ masks, const int* __restrict__ vbase,
                                                                  SparseLattice s, const int* __restrict__ counts,
                                                                  const int* __restrict__ tiles, int* __restrict__ triangles,
                                                                  long long capacity) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int corner[8], rows[6];
  const int mine = sparse_cell_triangles(flags, s, sparse_point(s, i), corner, rows);
  const int v[4] = {mine, 0, 0, 0};
  int total;
  const int before = tile_scan(v, total);
  if (!mine) return;
  long long row = scan_row(counts, tiles, before);
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int n_tri = rows[t] & 3;
    for (int k = 0; k < n_tri; ++k, ++row) {
      if (row >= capacity) return;
      int index[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        int c_lo, dir;
        tet_row_edge(rows[t], t, k, m, c_lo, dir);
        int owner = corner[0];
#pragma unroll
        for (int c = 1; c < 8; ++c) owner = c_lo == c ? corner[c] : owner;  // (selects: no indexed private array)
        index[m] = vbase[owner] + __popc(masks[owner] & ((1 << dir) - 1));
      }
      const bool swap = TET_ODD[t];
      triangles[row * 3 + 0] = index[0];
      triangles[row * 3 + 1] = swap ? index[2] : index[1];
      triangles[row * 3 + 2] = swap ? index[1] : index[2];
    }
  }
}

static bool sparse_mesh_sizes_ok(int64_t n_bricks, int32_t bx, int32_t by, int32_t bz) {
  return brick_dims_ok(bx, by, bz) && n_bricks >= 0 && n_bricks <= (long long)bx * by * bz && n_bricks <= SPARSE_MAX_BRICKS;
}

extern "C" int64_t mnerf_tsdf_mesh_sparse_workspace_bytes(int64_t n_bricks, int32_t bx, int32_t by, int32_t bz) {
  if (!sparse_mesh_sizes_ok(n_bricks, bx, by, bz)) return -1;
  return mesh_workspace(nullptr, n_bricks * BRICK_POINTS).bytes;
}

extern "C" int mnerf_tsdf_mesh_sparse(const float* sums, const float* weight, const int32_t* table, const int32_t* bricks, int64_t n_bricks,
                                      float origin_x, float origin_y, float origin_z, float voxel, int32_t nx, int32_t ny, int32_t nz,
                                      float min_weight, float* vertices, int64_t vertex_capacity, int32_t* triangles,
                                      int64_t triangle_capacity, int64_t* counts, void* workspace, void* stream) {
  const char* who = "mnerf_tsdf_mesh_sparse";
  MNERF_REQUIRE(grid_ok(origin_x, origin_y, origin_z, voxel, nx, ny, nz), MNERF_E_RANGE, "%s: grid %dx%dx%d of voxel %g at (%g, %g, %g)", who,
                nx, ny, nz, (double)voxel, (double)origin_x, (double)origin_y, (double)origin_z);
  const BrickGrid b = brick_grid(nx, ny, nz);
  MNERF_REQUIRE(brick_grid_ok(b), MNERF_E_RANGE, "%s: grid %dx%dx%d has 2^31 bricks or more", who, nx, ny, nz);
  if (const int rc = sparse_bricks_ok(who, n_bricks, b)) return rc;
  MNERF_REQUIRE(std::isfinite(min_weight) && min_weight > 0.0f, MNERF_E_RANGE, "%s: min_weight=%g must be finite and positive", who,
                (double)min_weight);
  MNERF_REQUIRE(vertex_capacity >= 0 && triangle_capacity >= 0, MNERF_E_RANGE, "%s: capacities %lld / %lld", who,
                (long long)vertex_capacity, (long long)triangle_capacity);
  if (n_bricks == 0) return MNERF_OK;
  MNERF_REQUIRE(sums && weight && counts && workspace, MNERF_E_NULL, "%s: NULL sums / weight / counts / workspace", who);
  MNERF_REQUIRE(table && bricks, MNERF_E_NULL, "%s: NULL table / bricks", who);
  MNERF_REQUIRE(vertex_capacity == 0 || vertices, MNERF_E_NULL, "%s: vertices is NULL", who);
  MNERF_REQUIRE(triangle_capacity == 0 || triangles, MNERF_E_NULL, "%s: triangles is NULL", who);
  MNERF_REQUIRE(mnerf_aligned16(sums) && mnerf_aligned16(vertices), MNERF_E_ALIGN, "%s: sums / vertices not 16B aligned", who);
  MNERF_REQUIRE((((uintptr_t)weight) & 3u) == 0 && (((uintptr_t)triangles) & 3u) == 0 && (((uintptr_t)workspace) & 3u) == 0 &&
                    (((uintptr_t)table) & 3u) == 0 && (((uintptr_t)bricks) & 3u) == 0 && (((uintptr_t)counts) & 7u) == 0,
                MNERF_E_ALIGN, "%s: weight / triangles / workspace / table / bricks / counts not aligned to 4 / 4 / 4 / 4 / 4 / 8 bytes", who);
  const MeshWorkspace w = mesh_workspace(workspace, n_bricks * BRICK_POINTS);
  long long* count = reinterpret_cast<long long*>(counts);
  const TsdfGrid g = {origin_x, origin_y, origin_z, voxel, nx, ny, nz};
  const SparseLattice s = {table, bricks, nx, ny, nz, b};
  const dim3 blocks((unsigned)w.vscan.blocks), threads(PC_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(smesh_flags_kernel, blocks, threads, 0, st, weight, sums, min_weight, s, w.flags);
  hipLaunchKernelGGL(smesh_vcount_kernel, blocks, threads, 0, st, w.flags, s, w.masks, w.vscan.counts);
  scan_enqueue(w.vscan, count, st);
  hipLaunchKernelGGL(smesh_vscatter_kernel, blocks, threads, 0, st, sums, weight, g, s, w.masks, w.vscan.counts, w.vscan.tiles, w.vbase,
                     vertices, (long long)vertex_capacity);
  hipLaunchKernelGGL(smesh_tcount_kernel, blocks, threads, 0, st, w.flags, s, w.tscan.counts);
  scan_enqueue(w.tscan, count + 1, st);
  hipLaunchKernelGGL(smesh_tscatter_kernel, blocks, threads, 0, st, w.flags, w.masks, w.vbase, s, w.tscan.counts, w.tscan.tiles, triangles,
                     (long long)triangle_capacity);
  return mnerf_check_launch(who);
}
#pragma clang fp contract(fast)
