// What the dense and the brick-sparse TSDF volume share (mesh.hip, tsdf_sparse.hip; include/mnerf.h "MESH EXPORT"): the grid, the
// integrator's per-view step - ONE device function, so that the sparse volume's mark and update agree with the dense update bit for
// bit - the tetrahedron table of the mesher and its flag bits.
// Include after fusion_common.hpp, under `#pragma clang fp contract(off)`.
#pragma once
#include <math.h>

#include "fusion_common.hpp"

struct TsdfGrid {
  float ox, oy, oz, voxel;
  int nx, ny, nz;
};

// the centre of voxel `index` along one axis: one FMA (index + 0.5 is exact)
__device__ __forceinline__ float voxel_centre(int index, float voxel, float origin) {
  return __builtin_fmaf((float)index + 0.5f, voxel, origin);
}

// what every view of a call shares
struct TsdfMaps {
  int height, width, legacy_coord;
  const float* __restrict__ depth;
  const float* __restrict__ opacity;
  const int* __restrict__ n_consistent;
  int min_consistent;
  float min_opacity, trunc;
};

// View j's update of the voxel centred at (px, py, pz), as include/mnerf.h states it: false = the view skips the voxel; true = it adds
// t to S, rgb[texel] to RGB and 1 to the weight.
__device__ __forceinline__ bool tsdf_view_step(const FusionCam& J, int j, const TsdfMaps& m, float px, float py, float pz, size_t& texel,
                                               float& t) {
  const float off = m.legacy_coord ? 0.0f : 0.5f;
  const long long n = (long long)m.height * m.width;
  float u, v, zc;
  fusion_project(J, px, py, pz, u, v, zc);
  if (!(zc > 0.0f)) return false;
  const float fx = floorf((u - off) + 0.5f), fy = floorf((v - off) + 0.5f);
  if (!(fx >= 0.0f && fx < (float)m.width && fy >= 0.0f && fy < (float)m.height)) return false;
  texel = (size_t)j * n + (size_t)((int)fy) * m.width + (int)fx;
  float z;
  if (!fusion_value(m.depth, m.opacity, texel, m.min_opacity, J.v.near_, J.v.far_, z)) return false;
  if (m.n_consistent && m.n_consistent[texel] < m.min_consistent) return false;
  const float sdf = z - zc;
  if (sdf < -m.trunc) return false;  // hidden behind the surface
  t = fminf(1.0f, sdf / m.trunc);
  return true;
}

static bool grid_ok(float ox, float oy, float oz, float voxel, int nx, int ny, int nz) {
  return std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz) && std::isfinite(voxel) && voxel > 0.0f && nx >= 0 && ny >= 0 &&
         nz >= 0;
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

// ------------------------------------------------------------------------------------------------ what the meshers share
constexpr unsigned char MF_VALID = 1, MF_INSIDE = 2, MF_CELL = 4;

__device__ __forceinline__ int tet_code(int cell, int t) {
  return (cell >> tet_corner(t, 0) & 1) | (cell >> tet_corner(t, 1) & 1) << 1 | (cell >> tet_corner(t, 2) & 1) << 2 |
         (cell >> tet_corner(t, 3) & 1) << 3;
}

// the table rows of the six tets of a cell whose corners' inside bits are `cell` (-1: no valid cell; 0: the tet emits nothing);
// returns the triangles the cell emits, their counts' sum
__device__ __forceinline__ int cell_rows(int cell, int rows[6]) {
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

// the corner codes of the ends of polygon vertex m of triangle k of tet t's table row: the owner's corner and the edge's direction
__device__ __forceinline__ void tet_row_edge(int row, int t, int k, int m, int& c_lo, int& dir) {
  const int edge = row >> (2 + 4 * (3 * k + m)) & 15;
  const int lo = edge >> 2, hi = edge & 3;
  int c_hi = 0;
  c_lo = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {  // (selects instead of an indexed table: tet_corner(t, q) is a constant where t is)
    c_lo = lo == q ? tet_corner(t, q) : c_lo;
    c_hi = hi == q ? tet_corner(t, q) : c_hi;
  }
  dir = (c_hi ^ c_lo) - 1;
}

// what bounds every index of a mesher below 2^31: at most 7 vertices per lattice point and 12 triangles per cell
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
