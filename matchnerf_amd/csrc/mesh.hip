// Mesh export (include/mnerf.h "MESH EXPORT"): TSDF fusion of rendered depth maps into a voxel volume, and marching tetrahedra over
// the Freudenthal split of its cells into a welded, indexed, coloured triangle mesh.
//
// Memory-bound kernels of one thread per voxel / lattice point, x fastest, 256 threads per workgroup:
//   tsdf_integrate_kernel   per voxel and view: one projection, one texel, a read-modify-write of five floats
//   mesh_flags_kernel       per lattice point: valid | inside | "the cell I am the origin of is valid", one byte
//   mesh_vcount / the scan (scan.hip) / mesh_vscatter   the 7-bit mask of live owned edges, the two-level scan of the
//                           workgroups' counts, each point's vertex base, the vertex rows
//   mesh_tcount / the scan / mesh_tscatter   the same over cells for the triangles
// No atomics anywhere: vertices and triangles come out in a defined order and two runs give the same bits.
#include <math.h>

#include "common.hpp"

// every operation rounds on its own; the FMAs are the explicit ones
#pragma clang fp contract(off)

#include "fusion_common.hpp"
#include "tsdf_common.hpp"

// ------------------------------------------------------------------------------------------------ integration
__global__ __launch_bounds__(PC_BLOCK) void tsdf_integrate_kernel(FusionCams cams, int n_views, int height, int width, int legacy_coord,
                                                                  const float* __restrict__ depth, const float* __restrict__ opacity,
                                                                  const int* __restrict__ n_consistent, int min_consistent,
                                                                  const float* __restrict__ rgb, float min_opacity, float trunc,
                                                                  TsdfGrid g, float* __restrict__ sums, float* __restrict__ weight) {
  const long long n_voxels = (long long)g.nx * g.ny * g.nz;
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_voxels) return;
  const int ix = (int)(i % g.nx), iy = (int)((i / g.nx) % g.ny), iz = (int)(i / ((long long)g.nx * g.ny));
  const float px = voxel_centre(ix, g.voxel, g.ox), py = voxel_centre(iy, g.voxel, g.oy), pz = voxel_centre(iz, g.voxel, g.oz);
  const TsdfMaps maps = {height, width, legacy_coord, depth, opacity, n_consistent, min_consistent, min_opacity, trunc};
  float4 acc = reinterpret_cast<const float4*>(sums)[i];
  float wsum = weight[i];
  for (int j = 0; j < n_views; ++j) {  // (wave-uniform: the cameras are read through scalar loads)
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

extern "C" int mnerf_tsdf_integrate(const mnerf_view* views, int32_t n_views, int32_t height, int32_t width, int32_t legacy_coord,
                                    const float* depth, const float* opacity, const int32_t* n_consistent, int32_t min_consistent,
                                    const float* rgb, float min_opacity, float trunc, float origin_x, float origin_y, float origin_z,
                                    float voxel, int32_t nx, int32_t ny, int32_t nz, float* sums, float* weight, void* stream) {
  MNERF_REQUIRE(n_views >= 1 && n_views <= MNERF_MAX_VIEWS, MNERF_E_RANGE, "mnerf_tsdf_integrate: n_views=%d outside 1..%d", n_views,
                MNERF_MAX_VIEWS);
  MNERF_REQUIRE(height >= 1 && width >= 1 && (long long)height * width < (1ll << 31), MNERF_E_RANGE, "mnerf_tsdf_integrate: maps %dx%d",
                height, width);
  MNERF_REQUIRE(std::isfinite(trunc) && trunc > 0.0f, MNERF_E_RANGE, "mnerf_tsdf_integrate: trunc=%g must be finite and positive",
                (double)trunc);
  MNERF_REQUIRE(!opacity || std::isfinite(min_opacity), MNERF_E_RANGE, "mnerf_tsdf_integrate: min_opacity=%g", (double)min_opacity);
  MNERF_REQUIRE(grid_ok(origin_x, origin_y, origin_z, voxel, nx, ny, nz), MNERF_E_RANGE,
                "mnerf_tsdf_integrate: grid %dx%dx%d of voxel %g at (%g, %g, %g)", nx, ny, nz, (double)voxel, (double)origin_x,
                (double)origin_y, (double)origin_z);
  const double n_voxels_d = (double)nx * (double)ny * (double)nz;  // exact below 2^53
  MNERF_REQUIRE(n_voxels_d < 2147483648.0, MNERF_E_RANGE, "mnerf_tsdf_integrate: grid %dx%dx%d has 2^31 voxels or more", nx, ny, nz);
  const long long n_voxels = (long long)nx * ny * nz;
  if (n_voxels == 0) return MNERF_OK;
  MNERF_REQUIRE(views, MNERF_E_NULL, "mnerf_tsdf_integrate: views is NULL");
  MNERF_REQUIRE(depth && rgb && sums && weight, MNERF_E_NULL, "mnerf_tsdf_integrate: NULL depth / rgb / sums / weight");
  MNERF_REQUIRE(mnerf_aligned16(sums), MNERF_E_ALIGN, "mnerf_tsdf_integrate: sums not 16B aligned");
  MNERF_REQUIRE((((uintptr_t)weight) & 3u) == 0, MNERF_E_ALIGN, "mnerf_tsdf_integrate: weight not 4B aligned");
  FusionCams cams = {};
  for (int k = 0; k < n_views; ++k)
    MNERF_REQUIRE(fusion_cam(views[k], &cams.cam[k]), MNERF_E_RANGE, "mnerf_tsdf_integrate: view %d has a singular intr or extr", k);
  const TsdfGrid g = {origin_x, origin_y, origin_z, voxel, nx, ny, nz};
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((n_voxels + PC_BLOCK - 1) / PC_BLOCK)), dim3(PC_BLOCK), 0, (hipStream_t)stream,
                     cams, n_views, height, width, legacy_coord ? 1 : 0, depth, opacity, n_consistent, min_consistent, rgb, min_opacity,
                     trunc, g, sums, weight);
  return mnerf_check_launch("mnerf_tsdf_integrate");
}

// ------------------------------------------------------------------------------------------------ mesher
__global__ __launch_bounds__(PC_BLOCK) void mesh_flags_kernel(const float* __restrict__ sums, const float* __restrict__ weight,
                                                              float min_weight, int nx, int ny, int nz,
                                                              unsigned char* __restrict__ flags) {
  const long long n = (long long)nx * ny * nz;
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int ix = (int)(i % nx), iy = (int)((i / nx) % ny), iz = (int)(i / ((long long)nx * ny));
  const float w = weight[i];
  unsigned char f = 0;
  if (w >= min_weight) {
    f = MF_VALID;
    if (sums[i * 4] / w < 0.0f) f |= MF_INSIDE;
    if (ix + 1 < nx && iy + 1 < ny && iz + 1 < nz) {
      bool all = true;
#pragma unroll
      for (int c = 1; c < 8; ++c) all &= weight[i + (c & 1) + (long long)(c >> 1 & 1) * nx + (long long)(c >> 2) * nx * ny] >= min_weight;
      if (all) f |= MF_CELL;
    }
  }
  flags[i] = f;
}

// the mask of the live edges that lattice point i owns: bit e - 1 for the edge to i + e, whose ends differ in sign and which a valid
// cell uses (the cells at i - f for the corners f disjoint from e)
__device__ __forceinline__ int live_edges(const unsigned char* __restrict__ flags, long long i, int nx, int ny, int nz) {
  const int ix = (int)(i % nx), iy = (int)((i / nx) % ny), iz = (int)(i / ((long long)nx * ny));
  const long long sy = nx, sz = (long long)nx * ny;
  int cells = 0;  // bit f: the cell at i - f exists and is valid
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    const int fx = f & 1, fy = f >> 1 & 1, fz = f >> 2;
    if (ix - fx >= 0 && iy - fy >= 0 && iz - fz >= 0 && (flags[i - fx - fy * sy - fz * sz] & MF_CELL)) cells |= 1 << f;
  }
  if (!cells) return 0;
  const int inside = flags[i] & MF_INSIDE;
  int mask = 0;
#pragma unroll
  for (int e = 1; e < 8; ++e) {
    const int ex = e & 1, ey = e >> 1 & 1, ez = e >> 2;
    int users = 0;
#pragma unroll
    for (int f = 0; f < 8; ++f)
      if (!(f & e)) users |= 1 << f;
    if (!(cells & users)) continue;  // (then i + e lies inside the grid: a cell holding both exists)
    if ((flags[i + ex + ey * sy + ez * sz] & MF_INSIDE) != inside) mask |= 1 << (e - 1);
  }
  return mask;
}

__global__ __launch_bounds__(PC_BLOCK) void mesh_vcount_kernel(const unsigned char* __restrict__ flags, int nx, int ny, int nz,
                                                               unsigned char* __restrict__ masks, int* __restrict__ counts) {
  const long long n = (long long)nx * ny * nz;
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int mask = 0;
  if (i < n) {
    mask = live_edges(flags, i, nx, ny, nz);
    masks[i] = (unsigned char)mask;
  }
  const int v[4] = {(int)__popc(mask), 0, 0, 0};
  int total;
  tile_scan(v, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void mesh_vscatter_kernel(const float* __restrict__ sums, const float* __restrict__ weight,
                                                                 TsdfGrid g, const unsigned char* __restrict__ masks,
                                                                 const int* __restrict__ counts, const int* __restrict__ tiles,
                                                                 int* __restrict__ vbase, float* __restrict__ vertices,
                                                                 long long capacity) {
  const long long n = (long long)g.nx * g.ny * g.nz;
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const int mask = i < n ? masks[i] : 0;
  const int v[4] = {(int)__popc(mask), 0, 0, 0};
  int total;
  const int before = tile_scan(v, total);
  if (i >= n) return;
  long long row = scan_row(counts, tiles, before);
  vbase[i] = (int)row;
  if (!mask) return;
  const int ix = (int)(i % g.nx), iy = (int)((i / g.nx) % g.ny), iz = (int)(i / ((long long)g.nx * g.ny));
  const float4 sa = reinterpret_cast<const float4*>(sums)[i];
  const float wa = weight[i];
  const float da = sa.x / wa, ra = sa.y / wa, ga = sa.z / wa, ba = sa.w / wa;
  const float ax = voxel_centre(ix, g.voxel, g.ox), ay = voxel_centre(iy, g.voxel, g.oy), az = voxel_centre(iz, g.voxel, g.oz);
#pragma unroll
  for (int e = 1; e < 8; ++e) {
    if (!(mask >> (e - 1) & 1)) continue;
    if (row >= capacity) return;
    const int ex = e & 1, ey = e >> 1 & 1, ez = e >> 2;
    const long long j = i + ex + (long long)ey * g.nx + (long long)ez * g.nx * g.ny;
    const float4 sb = reinterpret_cast<const float4*>(sums)[j];
    const float wb = weight[j];
    const float db = sb.x / wb, rb = sb.y / wb, gb = sb.z / wb, bb = sb.w / wb;
    const float bx = voxel_centre(ix + ex, g.voxel, g.ox), by = voxel_centre(iy + ey, g.voxel, g.oy),
                bz = voxel_centre(iz + ez, g.voxel, g.oz);
    const float s = da / (da - db);
    float4* out = reinterpret_cast<float4*>(vertices) + (size_t)row * 2;
    out[0] = make_float4(__builtin_fmaf(s, bx - ax, ax), __builtin_fmaf(s, by - ay, ay), __builtin_fmaf(s, bz - az, az),
                         __builtin_fmaf(s, wb - wa, wa));
    out[1] = make_float4(__builtin_fmaf(s, rb - ra, ra), __builtin_fmaf(s, gb - ga, ga), __builtin_fmaf(s, bb - ba, ba), 0.0f);
    ++row;
  }
}

// the inside bits of the 8 corners of the cell at i, or -1 where i is the origin of no valid cell
__device__ __forceinline__ int cell_code(const unsigned char* __restrict__ flags, long long i, long long n, int nx, int ny) {
  if (i >= n || !(flags[i] & MF_CELL)) return -1;
  int code = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (flags[i + (c & 1) + (long long)(c >> 1 & 1) * nx + (long long)(c >> 2) * nx * ny] & MF_INSIDE) code |= 1 << c;
  return code;
}

// the table rows of the six tets of the cell at i (0: the tet emits nothing); returns the triangles the cell emits, their counts' sum
__device__ __forceinline__ int cell_triangles(const unsigned char* __restrict__ flags, long long i, long long n, int nx, int ny,
                                              int rows[6]) {
  return cell_rows(cell_code(flags, i, n, nx, ny), rows);
}

__global__ __launch_bounds__(PC_BLOCK) void mesh_tcount_kernel(const unsigned char* __restrict__ flags, int nx, int ny, int nz,
                                                               int* __restrict__ counts) {
  const long long n = (long long)nx * ny * nz;
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int rows[6];
  const int v[4] = {cell_triangles(flags, i, n, nx, ny, rows), 0, 0, 0};
  int total;
  tile_scan(v, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void mesh_tscatter_kernel(const unsigned char* __restrict__ flags,
                                                                 const unsigned char* __restrict__ masks, const int* __restrict__ vbase,
                                                                 int nx, int ny, int nz, const int* __restrict__ counts,
                                                                 const int* __restrict__ tiles, int* __restrict__ triangles,
                                                                 long long capacity) {
  const long long n = (long long)nx * ny * nz;
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int rows[6];
  const int mine = cell_triangles(flags, i, n, nx, ny, rows);
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
        const long long owner = i + (c_lo & 1) + (long long)(c_lo >> 1 & 1) * nx + (long long)(c_lo >> 2) * nx * ny;
        index[m] = vbase[owner] + __popc(masks[owner] & ((1 << dir) - 1));
      }
      const bool swap = TET_ODD[t];
      triangles[row * 3 + 0] = index[0];
      triangles[row * 3 + 1] = swap ? index[2] : index[1];
      triangles[row * 3 + 2] = swap ? index[1] : index[2];
    }
  }
}

extern "C" int64_t mnerf_tsdf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (nx < 0 || ny < 0 || nz < 0) return -1;
  const double n = (double)nx * (double)ny * (double)nz;
  if (n > (double)MESH_MAX_POINTS) return -1;
  return mesh_workspace(nullptr, (long long)nx * ny * nz).bytes;
}

extern "C" int mnerf_tsdf_mesh(const float* sums, const float* weight, float origin_x, float origin_y, float origin_z, float voxel,
                               int32_t nx, int32_t ny, int32_t nz, float min_weight, float* vertices, int64_t vertex_capacity,
                               int32_t* triangles, int64_t triangle_capacity, int64_t* counts, void* workspace, void* stream) {
  MNERF_REQUIRE(grid_ok(origin_x, origin_y, origin_z, voxel, nx, ny, nz), MNERF_E_RANGE,
                "mnerf_tsdf_mesh: grid %dx%dx%d of voxel %g at (%g, %g, %g)", nx, ny, nz, (double)voxel, (double)origin_x, (double)origin_y,
                (double)origin_z);
  MNERF_REQUIRE((double)nx * (double)ny * (double)nz <= (double)MESH_MAX_POINTS, MNERF_E_RANGE,
                "mnerf_tsdf_mesh: grid %dx%dx%d has more than %lld lattice points", nx, ny, nz, MESH_MAX_POINTS);
  MNERF_REQUIRE(std::isfinite(min_weight) && min_weight > 0.0f, MNERF_E_RANGE, "mnerf_tsdf_mesh: min_weight=%g must be finite and positive",
                (double)min_weight);
  MNERF_REQUIRE(vertex_capacity >= 0 && triangle_capacity >= 0, MNERF_E_RANGE, "mnerf_tsdf_mesh: capacities %lld / %lld",
                (long long)vertex_capacity, (long long)triangle_capacity);
  const long long n = (long long)nx * ny * nz;
  if (n == 0) return MNERF_OK;
  MNERF_REQUIRE(sums && weight && counts && workspace, MNERF_E_NULL, "mnerf_tsdf_mesh: NULL sums / weight / counts / workspace");
  MNERF_REQUIRE(vertex_capacity == 0 || vertices, MNERF_E_NULL, "mnerf_tsdf_mesh: vertices is NULL");
  MNERF_REQUIRE(triangle_capacity == 0 || triangles, MNERF_E_NULL, "mnerf_tsdf_mesh: triangles is NULL");
  MNERF_REQUIRE(mnerf_aligned16(sums) && mnerf_aligned16(vertices), MNERF_E_ALIGN, "mnerf_tsdf_mesh: sums / vertices not 16B aligned");
  MNERF_REQUIRE((((uintptr_t)weight) & 3u) == 0 && (((uintptr_t)triangles) & 3u) == 0 && (((uintptr_t)workspace) & 3u) == 0 &&
                    (((uintptr_t)counts) & 7u) == 0,
                MNERF_E_ALIGN, "mnerf_tsdf_mesh: weight / triangles / workspace / counts not aligned to 4 / 4 / 4 / 8 bytes");
  const MeshWorkspace w = mesh_workspace(workspace, n);
  long long* count = reinterpret_cast<long long*>(counts);
  const TsdfGrid g = {origin_x, origin_y, origin_z, voxel, nx, ny, nz};
  const dim3 blocks((unsigned)w.vscan.blocks), threads(PC_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_flags_kernel, blocks, threads, 0, st, sums, weight, min_weight, nx, ny, nz, w.flags);
  hipLaunchKernelGGL(mesh_vcount_kernel, blocks, threads, 0, st, w.flags, nx, ny, nz, w.masks, w.vscan.counts);
  scan_enqueue(w.vscan, count, st);
  hipLaunchKernelGGL(mesh_vscatter_kernel, blocks, threads, 0, st, sums, weight, g, w.masks, w.vscan.counts, w.vscan.tiles, w.vbase,
                     vertices, (long long)vertex_capacity);
  hipLaunchKernelGGL(mesh_tcount_kernel, blocks, threads, 0, st, w.flags, nx, ny, nz, w.tscan.counts);
  scan_enqueue(w.tscan, count + 1, st);
  hipLaunchKernelGGL(mesh_tscatter_kernel, blocks, threads, 0, st, w.flags, w.masks, w.vbase, nx, ny, nz, w.tscan.counts, w.tscan.tiles,
                     triangles, (long long)triangle_capacity);
  return mnerf_check_launch("mnerf_tsdf_mesh");
}
#pragma clang fp contract(fast)
