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

struct TsdfGrid {
  float ox, oy, oz, voxel;
  int nx, ny, nz;
};

// the centre of voxel `index` along one axis: one FMA (index + 0.5 is exact)
__device__ __forceinline__ float voxel_centre(int index, float voxel, float origin) {
  return __builtin_fmaf((float)index + 0.5f, voxel, origin);
}

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
  const float off = legacy_coord ? 0.0f : 0.5f;
  const long long n = (long long)height * width;
  float4 acc = reinterpret_cast<const float4*>(sums)[i];
  float wsum = weight[i];
  for (int j = 0; j < n_views; ++j) {  // (wave-uniform: the cameras are read through scalar loads)
    const FusionCam& J = cams.cam[j];
    float u, v, zc;
    fusion_project(J, px, py, pz, u, v, zc);
    if (!(zc > 0.0f)) continue;
    const float fx = floorf((u - off) + 0.5f), fy = floorf((v - off) + 0.5f);
    if (!(fx >= 0.0f && fx < (float)width && fy >= 0.0f && fy < (float)height)) continue;
    const size_t texel = (size_t)j * n + (size_t)((int)fy) * width + (int)fx;
    float z;
    if (!fusion_value(depth, opacity, texel, min_opacity, J.v.near_, J.v.far_, z)) continue;
    if (n_consistent && n_consistent[texel] < min_consistent) continue;
    const float sdf = z - zc;
    if (sdf < -trunc) continue;  // hidden behind the surface
    const float t = fminf(1.0f, sdf / trunc);
    acc.x = acc.x + t;
    acc.y = acc.y + rgb[texel * 3 + 0];
    acc.z = acc.z + rgb[texel * 3 + 1];
    acc.w = acc.w + rgb[texel * 3 + 2];
    wsum = wsum + 1.0f;
  }
  reinterpret_cast<float4*>(sums)[i] = acc;
  weight[i] = wsum;
}

static bool grid_ok(float ox, float oy, float oz, float voxel, int nx, int ny, int nz) {
  return std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz) && std::isfinite(voxel) && voxel > 0.0f && nx >= 0 && ny >= 0 &&
         nz >= 0;
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

// ------------------------------------------------------------------------------------------------ the tetrahedron table
// A cell's corner c = x | y << 1 | z << 2.  Tet t of a cell is 000 -> +e_a -> +e_a + e_b -> 111 with (a, b) the first two axes of
// the permutations xyz xzy yxz yzx zxy zyx; the even permutations (tets 0, 3, 4) are positively oriented.  An edge direction is
// e - 1 for e = the (non-zero) corner difference.
constexpr int TET_A[6] = {0, 0, 1, 1, 2, 2};
constexpr int TET_B[6] = {1, 2, 0, 2, 0, 1};
constexpr int TET_ODD[6] = {0, 1, 1, 0, 0, 1};

__host__ __device__ constexpr int tet_corner(int t, int k) {  // corner code of vertex k of tet t
  return k == 0 ? 0 : k == 1 ? (1 << TET_A[t]) : k == 2 ? ((1 << TET_A[t]) | (1 << TET_B[t])) : 7;
}

// Case `code` (bit k: vertex k inside) of a POSITIVELY oriented tet -> bits 0-1 the triangle count, then six 4-bit polygon vertices
// (lo << 2 | hi: the tet edge between vertices lo < hi), three per triangle.  With I the inside and O the outside vertices, both
// ascending:  |I| = 1, I = {a}: the edges from a to the others ascending;  |I| = 3, O = {a}: the same;  |I| = 2, I = {a, b},
// O = {c, d}: the quad ac ad bd bc as the triangles (ac ad bd) (ac bd bc) - the diagonal ac-bd.  That order has its normal from the
// inside to the outside iff the permutation (I, O) of 0123 is even; an odd one swaps the last two vertices of every triangle (and so
// does an odd tet, at the use).
struct TetTable {
  unsigned int row[16];
};
constexpr unsigned int tet_edge(int p, int q) { return (unsigned int)(p < q ? (p << 2 | q) : (q << 2 | p)); }
constexpr TetTable make_tet_table() {
  TetTable t = {};
  for (int code = 0; code < 16; ++code) {
    int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0, inversions = 0;
    for (int k = 0; k < 4; ++k) {
      if (code >> k & 1) in[n_in++] = k;
      else out[n_out++] = k;
    }
    for (int i = 0; i < n_in; ++i)
      for (int o = 0; o < n_out; ++o) inversions += in[i] > out[o];
    unsigned int poly[6] = {};
    int n_tri = 0;
    if (n_in == 1 || n_in == 3) {
      const int a = n_in == 1 ? in[0] : out[0];
      const int* rest = n_in == 1 ? out : in;
      n_tri = 1;
      for (int k = 0; k < 3; ++k) poly[k] = tet_edge(a, rest[k]);
    } else if (n_in == 2) {
      n_tri = 2;
      const unsigned int ac = tet_edge(in[0], out[0]), ad = tet_edge(in[0], out[1]), bd = tet_edge(in[1], out[1]),
                         bc = tet_edge(in[1], out[0]);
      poly[0] = ac, poly[1] = ad, poly[2] = bd, poly[3] = ac, poly[4] = bd, poly[5] = bc;
    }
    if (inversions & 1)
      for (int k = 0; k < n_tri; ++k) {
        const unsigned int s = poly[3 * k + 1];
        poly[3 * k + 1] = poly[3 * k + 2];
        poly[3 * k + 2] = s;
      }
    unsigned int row = (unsigned int)n_tri;
    for (int k = 0; k < 6; ++k) row |= poly[k] << (2 + 4 * k);
    t.row[code] = row;
  }
  return t;
}
__constant__ const TetTable TET_TABLE = make_tet_table();

// ------------------------------------------------------------------------------------------------ mesher
constexpr unsigned char MF_VALID = 1, MF_INSIDE = 2, MF_CELL = 4;

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

__device__ __forceinline__ int tet_code(int cell, int t) {
  return (cell >> tet_corner(t, 0) & 1) | (cell >> tet_corner(t, 1) & 1) << 1 | (cell >> tet_corner(t, 2) & 1) << 2 |
         (cell >> tet_corner(t, 3) & 1) << 3;
}

// the table rows of the six tets of the cell at i (0: the tet emits nothing); returns the triangles the cell emits, their counts' sum
__device__ __forceinline__ int cell_triangles(const unsigned char* __restrict__ flags, long long i, long long n, int nx, int ny,
                                              int rows[6]) {
  const int cell = cell_code(flags, i, n, nx, ny);
  int mine = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) rows[t] = 0;
  if (cell > 0 && cell < 255) {  // (a branch, not six selects: most cells are empty or full, and whole waves skip the table)
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      rows[t] = (int)TET_TABLE.row[tet_code(cell, t)];
      mine += rows[t] & 3;
    }
  }
  return mine;
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
        const int edge = rows[t] >> (2 + 4 * (3 * k + m)) & 15;
        const int lo = edge >> 2, hi = edge & 3;
        int c_lo = 0, c_hi = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // (selects instead of an indexed table: tet_corner(t, q) is a constant here)
          c_lo = lo == q ? tet_corner(t, q) : c_lo;
          c_hi = hi == q ? tet_corner(t, q) : c_hi;
        }
        const long long owner = i + (c_lo & 1) + (long long)(c_lo >> 1 & 1) * nx + (long long)(c_lo >> 2) * nx * ny;
        const int dir = (c_hi ^ c_lo) - 1;
        index[m] = vbase[owner] + __popc(masks[owner] & ((1 << dir) - 1));
      }
      const bool swap = TET_ODD[t];
      triangles[row * 3 + 0] = index[0];
      triangles[row * 3 + 1] = swap ? index[2] : index[1];
      triangles[row * 3 + 2] = swap ? index[1] : index[2];
    }
  }
}

// what bounds every index of the mesher below 2^31: at most 7 vertices per lattice point and 12 triangles per cell
constexpr long long MESH_MAX_POINTS = ((1ll << 31) - 1) / 12;

struct MeshWorkspace {
  long long bytes;
  int* vbase;                   // int32 [n]: the first vertex row of every lattice point
  ScanScratch vscan, tscan;     // the scans over the points' vertices and the cells' triangles
  unsigned char *flags, *masks;  // uint8 [n] each
};
static MeshWorkspace mesh_workspace(void* workspace, long long n) {
  Carve c(workspace);
  MeshWorkspace w;
  w.vbase = c.array<int>((size_t)n);
  w.vscan = c.scan(n);
  w.tscan = c.scan(n);
  w.flags = c.array<unsigned char>((size_t)n);
  w.masks = c.array<unsigned char>((size_t)n);
  w.bytes = c.bytes();
  return w;
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
