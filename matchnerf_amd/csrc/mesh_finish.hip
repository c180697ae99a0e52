// Mesh finishing (include/mnerf.h "MESH FINISHING"): what turns the mesher's raw zero set - or any indexed triangle mesh in the
// project's layout - into a mesh one can use: the vertex -> corner adjacency, connected components and the removal of the small
// ones, Taubin smoothing of the positions, area-weighted vertex normals.
//
// Memory-bound streaming and gather kernels of one thread per vertex or per triangle, 256 threads per workgroup:
//   adj_count / finish_blocksum / finish_scan / finish_total / adj_offsets / adj_fill / adj_sort_class
//                           corners per vertex, the two-level scan of mesh.hip over them, the rows filled through a cursor, every
//                           row sorted by its own thread and classified
//   cc_init / cc_union / cc_flatten / cc_count / cc_largest / cc_keep
//                           a lock-free union-find over the triangles' edges, triangles per component, the keep bytes
//   compact_count / finish_scan / finish_total / compact_vertices / compact_triangles   the mesher's stable scan and scatter
//   smooth_step             one Jacobi step of the umbrella operator, ping-pong through the workspace
//   normals                 the corner sum of the triangles' cross products
// THE DETERMINISM RULE: two runs give the same bytes in every output.  No floating-point atomic anywhere: every float sum runs over
// a CSR row in ascending corner order inside one thread.  Integer atomics only where the final memory contents do not depend on
// their order: the corner counts and triangle counts (add), the largest component (max), the union-find's hooks (whose final roots
// are the components' smallest rows whatever the order), and the row fill, which is sorted afterwards.
#include <math.h>

#include "common.hpp"

// every operation rounds on its own; the FMAs are the explicit ones
#pragma clang fp contract(off)

#include "fusion_common.hpp"

// what keeps every corner id 3 t + k below 2^31
constexpr long long FINISH_MAX_VERTICES = (1ll << 31) - 1;
constexpr long long FINISH_MAX_TRIANGLES = ((1ll << 31) - 1) / 3;
constexpr unsigned char VC_BOUNDARY = 0, VC_INTERIOR = 1;

__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned int)v < (unsigned int)n; }

// ------------------------------------------------------------------------------------------------ the two-level scan
// values[n], one per thread -> the workgroups' totals
__global__ __launch_bounds__(PC_BLOCK) void finish_blocksum_kernel(const int* __restrict__ values, int n, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const int v[4] = {i < n ? values[i] : 0, 0, 0, 0};
  int total;
  tile_scan(v, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// the mesher's two scans (mesh.hip): the workgroups' counts in tiles of 1024, then the tiles' totals and the grand total
__global__ __launch_bounds__(PC_BLOCK) void finish_scan_kernel(int* __restrict__ counts, int n_blocks, int* __restrict__ tiles) {
  const long long first = (long long)blockIdx.x * PC_TILE + threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = first + k < n_blocks ? counts[first + k] : 0;
  int total;
  int p = tile_scan(v, total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (first + k < n_blocks) counts[first + k] = p;
    p += v[k];
  }
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void finish_total_kernel(int* __restrict__ tiles, int n_tiles, long long* __restrict__ count) {
  int carry = 0;
  for (int begin = 0; begin < n_tiles; begin += PC_TILE) {
    const int first = begin + threadIdx.x * 4;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = first + k < n_tiles ? tiles[first + k] : 0;
    int total;
    int p = carry + tile_scan(v, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (first + k < n_tiles) tiles[first + k] = p;
      p += v[k];
    }
    carry += total;
  }
  if (threadIdx.x == 0) *count = (long long)carry;
}

struct FinishScan {  // the scratch of one scan over n elements: int32 [blocks] | int32 [tiles]
  long long blocks, tiles;
};
static FinishScan finish_scan(long long n) {
  FinishScan s;
  s.blocks = (n + PC_BLOCK - 1) / PC_BLOCK;
  s.tiles = (s.blocks + PC_TILE - 1) / PC_TILE;
  return s;
}

// ------------------------------------------------------------------------------------------------ 1. adjacency
__global__ __launch_bounds__(PC_BLOCK) void adj_zero_kernel(int* __restrict__ offsets, int n_vertices) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i <= n_vertices) offsets[i] = 0;
}

__global__ __launch_bounds__(PC_BLOCK) void adj_count_kernel(const int* __restrict__ triangles, long long n_corners, int n_vertices,
                                                             int* __restrict__ offsets) {
  const long long c = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (c >= n_corners) return;
  const int v = triangles[c];
  if (in_range(v, n_vertices)) atomicAdd(&offsets[v], 1);
}

// offsets[v]: the count -> the exclusive prefix; cursor[v] = the same; offsets[V] = the total
__global__ __launch_bounds__(PC_BLOCK) void adj_offsets_kernel(int* __restrict__ offsets, int n_vertices, const int* __restrict__ counts,
                                                               const int* __restrict__ tiles, int* __restrict__ cursor) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const int mine = i < n_vertices ? offsets[i] : 0;
  const int v[4] = {mine, 0, 0, 0};
  int total;
  const int before = tile_scan(v, total);
  if (i >= n_vertices) return;
  const int first = tiles[blockIdx.x / PC_TILE] + counts[blockIdx.x] + before;
  offsets[i] = first;
  cursor[i] = first;
  if (i == n_vertices - 1) offsets[n_vertices] = first + mine;
}

__global__ __launch_bounds__(PC_BLOCK) void adj_fill_kernel(const int* __restrict__ triangles, long long n_corners, int n_vertices,
                                                            int* __restrict__ cursor, int* __restrict__ corners) {
  const long long c = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (c >= n_corners) return;
  const int v = triangles[c];
  if (in_range(v, n_vertices)) corners[atomicAdd(&cursor[v], 1)] = (int)c;  // (a slot of v's row: the row is sorted below)
}

// the vertex after (step 1) or before (step 2) corner c in its triangle
__device__ __forceinline__ int corner_vertex(const int* __restrict__ triangles, int c, int step) {
  const int t = c / 3, k = c - 3 * t;
  const int m = k + step;
  return triangles[3 * t + (m >= 3 ? m - 3 : m)];
}

__global__ __launch_bounds__(PC_BLOCK) void adj_sort_class_kernel(const int* __restrict__ triangles, const int* __restrict__ offsets,
                                                                  int n_vertices, int* __restrict__ corners,
                                                                  unsigned char* __restrict__ vclass) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const int begin = offsets[i], end = offsets[i + 1];
  for (int a = begin + 1; a < end; ++a) {  // insertion sort in place: rows are short, and any length works
    const int key = corners[a];
    int b = a - 1;
    while (b >= begin && corners[b] > key) {
      corners[b + 1] = corners[b];
      --b;
    }
    corners[b + 1] = key;
  }
  // interior iff every neighbour is the `next` vertex of exactly one corner of the row and the `prev` vertex of exactly one
  bool interior = end > begin;
  for (int a = begin; a < end && interior; ++a) {
    const int next = corner_vertex(triangles, corners[a], 1), prev = corner_vertex(triangles, corners[a], 2);
    if (!in_range(next, n_vertices) || !in_range(prev, n_vertices)) {
      interior = false;
      break;
    }
    int next_as_next = 0, next_as_prev = 0, prev_as_next = 0, prev_as_prev = 0;
    for (int b = begin; b < end; ++b) {
      const int n2 = corner_vertex(triangles, corners[b], 1), p2 = corner_vertex(triangles, corners[b], 2);
      next_as_next += n2 == next;
      next_as_prev += p2 == next;
      prev_as_next += n2 == prev;
      prev_as_prev += p2 == prev;
    }
    interior = next_as_next == 1 && next_as_prev == 1 && prev_as_next == 1 && prev_as_prev == 1;
  }
  vclass[i] = interior ? VC_INTERIOR : VC_BOUNDARY;
}

struct FinishWorkspace {
  long long bytes;
  size_t head;                                  // int64 [2]: totals of the scans / the largest component
  size_t per_vertex, vcounts, vtiles, tcounts, ttiles;  // int32 [V] | [Bv] | [Tv] | [Bt] | [Tt]   (adjacency, components, compact)
  size_t ping;                                  // fp32 [V][8], 16-byte aligned (smooth) - shares the bytes of the above
  FinishScan sv, st;
};
static FinishWorkspace finish_workspace(long long n_vertices, long long n_triangles) {
  FinishWorkspace w = {};
  if (n_vertices == 0) return w;
  w.sv = finish_scan(n_vertices);
  w.st = finish_scan(n_triangles);
  w.head = 0;
  w.per_vertex = 16;
  w.vcounts = w.per_vertex + 4 * (size_t)n_vertices;
  w.vtiles = w.vcounts + 4 * (size_t)w.sv.blocks;
  w.tcounts = w.vtiles + 4 * (size_t)w.sv.tiles;
  w.ttiles = w.tcounts + 4 * (size_t)w.st.blocks;
  const size_t integers = w.ttiles + 4 * (size_t)w.st.tiles;
  w.ping = 16;
  const size_t floats = w.ping + 32 * (size_t)n_vertices;
  w.bytes = (long long)(((integers > floats ? integers : floats) + 15) & ~(size_t)15);
  return w;
}

static bool finish_sizes_ok(int64_t n_vertices, int64_t n_triangles) {
  return n_vertices >= 0 && n_triangles >= 0 && n_vertices <= FINISH_MAX_VERTICES && n_triangles <= FINISH_MAX_TRIANGLES;
}

extern "C" int64_t mnerf_mesh_finish_workspace_bytes(int64_t n_vertices, int64_t n_triangles) {
  if (!finish_sizes_ok(n_vertices, n_triangles)) return -1;
  return finish_workspace(n_vertices, n_triangles).bytes;
}

static inline bool aligned_to(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
static inline unsigned int blocks_of(long long n) { return (unsigned int)((n + PC_BLOCK - 1) / PC_BLOCK); }

extern "C" int mnerf_mesh_adjacency(const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, int32_t* offsets, int32_t* corners,
                                    uint8_t* vertex_class, void* workspace, void* stream) {
  MNERF_REQUIRE(finish_sizes_ok(n_vertices, n_triangles), MNERF_E_RANGE, "mnerf_mesh_adjacency: %lld vertices / %lld triangles",
                (long long)n_vertices, (long long)n_triangles);
  if (n_vertices == 0) return MNERF_OK;
  MNERF_REQUIRE(offsets && vertex_class && workspace, MNERF_E_NULL, "mnerf_mesh_adjacency: NULL offsets / vertex_class / workspace");
  MNERF_REQUIRE(n_triangles == 0 || (triangles && corners), MNERF_E_NULL, "mnerf_mesh_adjacency: NULL triangles / corners");
  MNERF_REQUIRE(aligned_to(triangles, 4) && aligned_to(offsets, 4) && aligned_to(corners, 4), MNERF_E_ALIGN,
                "mnerf_mesh_adjacency: triangles / offsets / corners not 4B aligned");
  MNERF_REQUIRE(mnerf_aligned16(workspace), MNERF_E_ALIGN, "mnerf_mesh_adjacency: workspace not 16B aligned");
  const FinishWorkspace w = finish_workspace(n_vertices, n_triangles);
  char* base = static_cast<char*>(workspace);
  long long* total = reinterpret_cast<long long*>(base + w.head);
  int* cursor = reinterpret_cast<int*>(base + w.per_vertex);
  int* vcounts = reinterpret_cast<int*>(base + w.vcounts);
  int* vtiles = reinterpret_cast<int*>(base + w.vtiles);
  const int nv = (int)n_vertices;
  const long long n_corners = 3 * (long long)n_triangles;
  const dim3 threads(PC_BLOCK), vblocks(blocks_of(n_vertices)), cblocks(blocks_of(n_corners));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adj_zero_kernel, dim3(blocks_of(n_vertices + 1)), threads, 0, st, offsets, nv);
  if (n_corners) hipLaunchKernelGGL(adj_count_kernel, cblocks, threads, 0, st, triangles, n_corners, nv, offsets);
  hipLaunchKernelGGL(finish_blocksum_kernel, vblocks, threads, 0, st, offsets, nv, vcounts);
  hipLaunchKernelGGL(finish_scan_kernel, dim3((unsigned)w.sv.tiles), threads, 0, st, vcounts, (int)w.sv.blocks, vtiles);
  hipLaunchKernelGGL(finish_total_kernel, dim3(1), threads, 0, st, vtiles, (int)w.sv.tiles, total);
  hipLaunchKernelGGL(adj_offsets_kernel, vblocks, threads, 0, st, offsets, nv, vcounts, vtiles, cursor);
  if (n_corners) hipLaunchKernelGGL(adj_fill_kernel, cblocks, threads, 0, st, triangles, n_corners, nv, cursor, corners);
  hipLaunchKernelGGL(adj_sort_class_kernel, vblocks, threads, 0, st, triangles, offsets, nv, corners, vertex_class);
  return mnerf_check_launch("mnerf_mesh_adjacency");
}

// ------------------------------------------------------------------------------------------------ 2. components
// The union-find forest lives in `labels`: parent[v] <= v always.  A root is its own parent.
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// TERMINATION: every store to parent[] writes a value that is <= the one it replaces (cc_init writes v; a hook writes b < a over a;
// the flatten writes an ancestor), so a parent chain is strictly decreasing until it reaches a root: the walk takes at most x steps.
__device__ __forceinline__ int cc_find(const int* parent, int x) {
  for (;;) {
    const int p = cc_load(parent + x);
    if (p >= x) return x;  // (== x: a root)
    x = p;
  }
}

// Hook the larger root under the smaller.  TERMINATION: the compare-and-swap fails only if parent[a] is no longer a, and it only
// ever changes to something smaller: some root strictly decreased.  The sum of all parents is a non-negative integer that every
// failure witnesses a decrease of, so the number of failures over the whole launch is bounded by its initial value; every other
// pass through the loop ends it.
__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return;
    a = old;  // the smaller parent somebody else gave it
  }
}

__global__ __launch_bounds__(PC_BLOCK) void cc_init_kernel(int* __restrict__ parent, int* __restrict__ tri_count, int n_vertices,
                                                           int* __restrict__ largest) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i == 0) *largest = 0;
  if (i >= n_vertices) return;
  parent[i] = (int)i;
  tri_count[i] = 0;
}

__device__ __forceinline__ bool triangle_ok(const int* __restrict__ triangles, long long t, int n_vertices, int& a, int& b, int& c) {
  a = triangles[3 * t], b = triangles[3 * t + 1], c = triangles[3 * t + 2];
  return in_range(a, n_vertices) && in_range(b, n_vertices) && in_range(c, n_vertices);
}

__global__ __launch_bounds__(PC_BLOCK) void cc_union_kernel(const int* __restrict__ triangles, long long n_triangles, int n_vertices,
                                                            int* parent) {
  const long long t = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (t >= n_triangles) return;
  int a, b, c;
  if (!triangle_ok(triangles, t, n_vertices, a, b, c)) return;
  cc_unite(parent, a, b);
  cc_unite(parent, a, c);
}

// parent[v] <- its root.  Roots do not change in this launch, and every value written is an ancestor of the one it replaces, so
// concurrent walks stay on decreasing chains to the same roots.
__global__ __launch_bounds__(PC_BLOCK) void cc_flatten_kernel(int* parent, int n_vertices) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  __hip_atomic_store(parent + i, cc_find(parent, (int)i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(PC_BLOCK) void cc_count_kernel(const int* __restrict__ triangles, long long n_triangles, int n_vertices,
                                                            const int* __restrict__ labels, int* __restrict__ tri_count) {
  const long long t = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (t >= n_triangles) return;
  int a, b, c;
  if (triangle_ok(triangles, t, n_vertices, a, b, c)) atomicAdd(&tri_count[labels[a]], 1);
}

__global__ __launch_bounds__(PC_BLOCK) void cc_largest_kernel(const int* __restrict__ tri_count, int n_vertices, int* __restrict__ largest) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const int n = tri_count[i];  // (non-zero at the components' roots only)
  if (n > 0) atomicMax(largest, n);
}

__global__ __launch_bounds__(PC_BLOCK) void cc_keep_kernel(const int* __restrict__ labels, const int* __restrict__ tri_count, int n_vertices,
                                                           const int* __restrict__ largest, long long min_triangles, double min_fraction,
                                                           unsigned char* __restrict__ keep) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const int n = tri_count[labels[i]];
  keep[i] = (long long)n >= min_triangles && (double)n >= min_fraction * (double)*largest;
}

extern "C" int mnerf_mesh_components(const int32_t* triangles, int64_t n_vertices, int64_t n_triangles, int64_t min_triangles,
                                     double min_fraction, int32_t* labels, uint8_t* keep, void* workspace, void* stream) {
  MNERF_REQUIRE(finish_sizes_ok(n_vertices, n_triangles), MNERF_E_RANGE, "mnerf_mesh_components: %lld vertices / %lld triangles",
                (long long)n_vertices, (long long)n_triangles);
  MNERF_REQUIRE(min_triangles >= 0, MNERF_E_RANGE, "mnerf_mesh_components: min_triangles=%lld", (long long)min_triangles);
  MNERF_REQUIRE(std::isfinite(min_fraction) && min_fraction >= 0.0 && min_fraction <= 1.0, MNERF_E_RANGE,
                "mnerf_mesh_components: min_fraction=%g outside [0, 1]", min_fraction);
  if (n_vertices == 0) return MNERF_OK;
  MNERF_REQUIRE(labels && keep && workspace, MNERF_E_NULL, "mnerf_mesh_components: NULL labels / keep / workspace");
  MNERF_REQUIRE(n_triangles == 0 || triangles, MNERF_E_NULL, "mnerf_mesh_components: triangles is NULL");
  MNERF_REQUIRE(aligned_to(triangles, 4) && aligned_to(labels, 4), MNERF_E_ALIGN, "mnerf_mesh_components: triangles / labels not 4B aligned");
  MNERF_REQUIRE(mnerf_aligned16(workspace), MNERF_E_ALIGN, "mnerf_mesh_components: workspace not 16B aligned");
  const FinishWorkspace w = finish_workspace(n_vertices, n_triangles);
  char* base = static_cast<char*>(workspace);
  int* largest = reinterpret_cast<int*>(base + w.head);
  int* tri_count = reinterpret_cast<int*>(base + w.per_vertex);
  const int nv = (int)n_vertices;
  const dim3 threads(PC_BLOCK), vblocks(blocks_of(n_vertices)), tblocks(blocks_of(n_triangles));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_init_kernel, vblocks, threads, 0, st, labels, tri_count, nv, largest);
  if (n_triangles) hipLaunchKernelGGL(cc_union_kernel, tblocks, threads, 0, st, triangles, (long long)n_triangles, nv, labels);
  hipLaunchKernelGGL(cc_flatten_kernel, vblocks, threads, 0, st, labels, nv);
  if (n_triangles) hipLaunchKernelGGL(cc_count_kernel, tblocks, threads, 0, st, triangles, (long long)n_triangles, nv, labels, tri_count);
  hipLaunchKernelGGL(cc_largest_kernel, vblocks, threads, 0, st, tri_count, nv, largest);
  hipLaunchKernelGGL(cc_keep_kernel, vblocks, threads, 0, st, labels, tri_count, nv, largest, (long long)min_triangles, min_fraction, keep);
  return mnerf_check_launch("mnerf_mesh_components");
}

// ------------------------------------------------------------------------------------------------ 3. compaction
__device__ __forceinline__ bool triangle_kept(const int* __restrict__ triangles, long long t, long long n_triangles, int n_vertices,
                                              const unsigned char* __restrict__ keep, int& a, int& b, int& c) {
  return t < n_triangles && triangle_ok(triangles, t, n_vertices, a, b, c) && keep[a];
}

__global__ __launch_bounds__(PC_BLOCK) void compact_vcount_kernel(const unsigned char* __restrict__ keep, int n_vertices,
                                                                  int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int total;
  block_prefix(i < n_vertices && keep[i], total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void compact_tcount_kernel(const int* __restrict__ triangles, long long n_triangles, int n_vertices,
                                                                  const unsigned char* __restrict__ keep, int* __restrict__ counts) {
  const long long t = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int a, b, c, total;
  block_prefix(triangle_kept(triangles, t, n_triangles, n_vertices, keep, a, b, c), total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void compact_vertices_kernel(const float* __restrict__ vertices, const unsigned char* __restrict__ keep,
                                                                    int n_vertices, const int* __restrict__ counts,
                                                                    const int* __restrict__ tiles, int* __restrict__ new_row,
                                                                    float* __restrict__ out, long long capacity) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const bool kept = i < n_vertices && keep[i];
  int total;
  const int before = block_prefix(kept, total);
  if (i >= n_vertices) return;
  const long long row = (long long)tiles[blockIdx.x / PC_TILE] + counts[blockIdx.x] + before;
  new_row[i] = kept ? (int)row : -1;
  if (!kept || row >= capacity) return;
  const float4* src = reinterpret_cast<const float4*>(vertices) + (size_t)i * 2;
  float4* dst = reinterpret_cast<float4*>(out) + (size_t)row * 2;
  dst[0] = src[0];
  dst[1] = src[1];
}

__global__ __launch_bounds__(PC_BLOCK) void compact_triangles_kernel(const int* __restrict__ triangles, long long n_triangles,
                                                                     int n_vertices, const unsigned char* __restrict__ keep,
                                                                     const int* __restrict__ new_row, const int* __restrict__ counts,
                                                                     const int* __restrict__ tiles, int* __restrict__ out,
                                                                     long long capacity) {
  const long long t = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int a = 0, b = 0, c = 0, total;
  const bool kept = triangle_kept(triangles, t, n_triangles, n_vertices, keep, a, b, c);
  const int before = block_prefix(kept, total);
  if (!kept) return;
  const long long row = (long long)tiles[blockIdx.x / PC_TILE] + counts[blockIdx.x] + before;
  if (row >= capacity) return;
  out[row * 3 + 0] = new_row[a];
  out[row * 3 + 1] = new_row[b];
  out[row * 3 + 2] = new_row[c];
}

extern "C" int mnerf_mesh_compact(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles,
                                  const uint8_t* keep, float* vertices_out, int64_t vertex_capacity, int32_t* triangles_out,
                                  int64_t triangle_capacity, int64_t* counts, void* workspace, void* stream) {
  MNERF_REQUIRE(finish_sizes_ok(n_vertices, n_triangles), MNERF_E_RANGE, "mnerf_mesh_compact: %lld vertices / %lld triangles",
                (long long)n_vertices, (long long)n_triangles);
  MNERF_REQUIRE(vertex_capacity >= 0 && triangle_capacity >= 0, MNERF_E_RANGE, "mnerf_mesh_compact: capacities %lld / %lld",
                (long long)vertex_capacity, (long long)triangle_capacity);
  if (n_vertices == 0) return MNERF_OK;
  MNERF_REQUIRE(vertices && keep && counts && workspace, MNERF_E_NULL, "mnerf_mesh_compact: NULL vertices / keep / counts / workspace");
  MNERF_REQUIRE(n_triangles == 0 || triangles, MNERF_E_NULL, "mnerf_mesh_compact: triangles is NULL");
  MNERF_REQUIRE(vertex_capacity == 0 || vertices_out, MNERF_E_NULL, "mnerf_mesh_compact: vertices_out is NULL");
  MNERF_REQUIRE(triangle_capacity == 0 || n_triangles == 0 || triangles_out, MNERF_E_NULL, "mnerf_mesh_compact: triangles_out is NULL");
  MNERF_REQUIRE(mnerf_aligned16(vertices) && mnerf_aligned16(vertices_out) && mnerf_aligned16(workspace), MNERF_E_ALIGN,
                "mnerf_mesh_compact: vertices / vertices_out / workspace not 16B aligned");
  MNERF_REQUIRE(aligned_to(triangles, 4) && aligned_to(triangles_out, 4) && aligned_to(counts, 8), MNERF_E_ALIGN,
                "mnerf_mesh_compact: triangles / triangles_out / counts not aligned to 4 / 4 / 8 bytes");
  const FinishWorkspace w = finish_workspace(n_vertices, n_triangles);
  char* base = static_cast<char*>(workspace);
  int* new_row = reinterpret_cast<int*>(base + w.per_vertex);
  int* vcounts = reinterpret_cast<int*>(base + w.vcounts);
  int* vtiles = reinterpret_cast<int*>(base + w.vtiles);
  int* tcounts = reinterpret_cast<int*>(base + w.tcounts);
  int* ttiles = reinterpret_cast<int*>(base + w.ttiles);
  long long* count = reinterpret_cast<long long*>(counts);
  const int nv = (int)n_vertices;
  const long long nt = (long long)n_triangles;
  const dim3 threads(PC_BLOCK), vblocks(blocks_of(n_vertices)), tblocks(blocks_of(n_triangles));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(compact_vcount_kernel, vblocks, threads, 0, st, keep, nv, vcounts);
  hipLaunchKernelGGL(finish_scan_kernel, dim3((unsigned)w.sv.tiles), threads, 0, st, vcounts, (int)w.sv.blocks, vtiles);
  hipLaunchKernelGGL(finish_total_kernel, dim3(1), threads, 0, st, vtiles, (int)w.sv.tiles, count);
  hipLaunchKernelGGL(compact_vertices_kernel, vblocks, threads, 0, st, vertices, keep, nv, vcounts, vtiles, new_row, vertices_out,
                     (long long)vertex_capacity);
  if (nt) {
    hipLaunchKernelGGL(compact_tcount_kernel, tblocks, threads, 0, st, triangles, nt, nv, keep, tcounts);
    hipLaunchKernelGGL(finish_scan_kernel, dim3((unsigned)w.st.tiles), threads, 0, st, tcounts, (int)w.st.blocks, ttiles);
  }
  hipLaunchKernelGGL(finish_total_kernel, dim3(1), threads, 0, st, ttiles, (int)w.st.tiles, count + 1);
  if (nt)
    hipLaunchKernelGGL(compact_triangles_kernel, tblocks, threads, 0, st, triangles, nt, nv, keep, new_row, tcounts, ttiles, triangles_out,
                       (long long)triangle_capacity);
  return mnerf_check_launch("mnerf_mesh_compact");
}

// ------------------------------------------------------------------------------------------------ 4. smoothing
// one Jacobi step p <- p + factor (m - p) on the interior vertices; every other vertex and every other field is copied
__global__ __launch_bounds__(PC_BLOCK) void smooth_step_kernel(const float* src, const int* __restrict__ triangles,
                                                               const int* __restrict__ offsets, const int* __restrict__ corners,
                                                               const unsigned char* __restrict__ vclass, int n_vertices, float factor,
                                                               float* dst) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const float4* rows = reinterpret_cast<const float4*>(src);
  float4 p = rows[(size_t)i * 2];
  const float4 q = rows[(size_t)i * 2 + 1];
  if (factor != 0.0f && vclass[i] == VC_INTERIOR) {
    const int begin = offsets[i], end = offsets[i + 1];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int a = begin; a < end; ++a) {  // (an interior vertex's neighbours lie inside the buffer: adj_sort_class_kernel)
      const int c = corners[a];
      const float4 pn = rows[(size_t)corner_vertex(triangles, c, 1) * 2], pp = rows[(size_t)corner_vertex(triangles, c, 2) * 2];
      sx = sx + (pn.x + pp.x);
      sy = sy + (pn.y + pp.y);
      sz = sz + (pn.z + pp.z);
    }
    const float d = (float)(2 * (long long)(end - begin));
    p.x = __builtin_fmaf(factor, sx / d - p.x, p.x);
    p.y = __builtin_fmaf(factor, sy / d - p.y, p.y);
    p.z = __builtin_fmaf(factor, sz / d - p.z, p.z);
  }
  float4* out = reinterpret_cast<float4*>(dst);
  out[(size_t)i * 2] = p;
  out[(size_t)i * 2 + 1] = q;
}

extern "C" int mnerf_mesh_smooth(const float* vertices_in, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                 const int32_t* offsets, const int32_t* corners, const uint8_t* vertex_class, int32_t iterations,
                                 float lambda, float mu, float* vertices_out, void* workspace, void* stream) {
  MNERF_REQUIRE(finish_sizes_ok(n_vertices, n_triangles), MNERF_E_RANGE, "mnerf_mesh_smooth: %lld vertices / %lld triangles",
                (long long)n_vertices, (long long)n_triangles);
  MNERF_REQUIRE(iterations >= 0, MNERF_E_RANGE, "mnerf_mesh_smooth: iterations=%d", iterations);
  MNERF_REQUIRE(lambda > 0.0f && lambda <= 1.0f, MNERF_E_RANGE, "mnerf_mesh_smooth: lambda=%g outside (0, 1]", (double)lambda);
  MNERF_REQUIRE(std::isfinite(mu) && mu <= 0.0f, MNERF_E_RANGE, "mnerf_mesh_smooth: mu=%g must be finite and <= 0", (double)mu);
  if (n_vertices == 0) return MNERF_OK;
  MNERF_REQUIRE(vertices_in && vertices_out && offsets && vertex_class && workspace, MNERF_E_NULL,
                "mnerf_mesh_smooth: NULL vertices_in / vertices_out / offsets / vertex_class / workspace");
  MNERF_REQUIRE(n_triangles == 0 || (triangles && corners), MNERF_E_NULL, "mnerf_mesh_smooth: NULL triangles / corners");
  MNERF_REQUIRE(mnerf_aligned16(vertices_in) && mnerf_aligned16(vertices_out) && mnerf_aligned16(workspace), MNERF_E_ALIGN,
                "mnerf_mesh_smooth: vertices_in / vertices_out / workspace not 16B aligned");
  MNERF_REQUIRE(aligned_to(triangles, 4) && aligned_to(offsets, 4) && aligned_to(corners, 4), MNERF_E_ALIGN,
                "mnerf_mesh_smooth: triangles / offsets / corners not 4B aligned");
  const FinishWorkspace w = finish_workspace(n_vertices, n_triangles);
  float* ping = reinterpret_cast<float*>(static_cast<char*>(workspace) + w.ping);
  const int nv = (int)n_vertices;
  const dim3 threads(PC_BLOCK), vblocks(blocks_of(n_vertices));
  hipStream_t st = (hipStream_t)stream;
  if (iterations == 0) {  // a factor of 0 copies every row
    if (vertices_out != vertices_in)
      hipLaunchKernelGGL(smooth_step_kernel, vblocks, threads, 0, st, vertices_in, triangles, offsets, corners, vertex_class, nv, 0.0f,
                         vertices_out);
    return mnerf_check_launch("mnerf_mesh_smooth");
  }
  const float* src = vertices_in;
  for (int it = 0; it < iterations; ++it) {
    hipLaunchKernelGGL(smooth_step_kernel, vblocks, threads, 0, st, src, triangles, offsets, corners, vertex_class, nv, lambda, ping);
    hipLaunchKernelGGL(smooth_step_kernel, vblocks, threads, 0, st, (const float*)ping, triangles, offsets, corners, vertex_class, nv, mu,
                       vertices_out);
    src = vertices_out;
  }
  return mnerf_check_launch("mnerf_mesh_smooth");
}

// ------------------------------------------------------------------------------------------------ 5. normals
__global__ __launch_bounds__(PC_BLOCK) void normals_kernel(const float* __restrict__ vertices, const int* __restrict__ triangles,
                                                           const int* __restrict__ offsets, const int* __restrict__ corners,
                                                           int n_vertices, float* __restrict__ normals) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const float4* rows = reinterpret_cast<const float4*>(vertices);
  const int begin = offsets[i], end = offsets[i + 1];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, twice_area = 0.0f;
  for (int k = begin; k < end; ++k) {
    int a, b, c;
    if (!triangle_ok(triangles, corners[k] / 3, n_vertices, a, b, c)) continue;
    const float4 p0 = rows[(size_t)a * 2], p1 = rows[(size_t)b * 2], p2 = rows[(size_t)c * 2];
    const float ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
    const float vx = p2.x - p0.x, vy = p2.y - p0.y, vz = p2.z - p0.z;
    const float cx = __builtin_fmaf(uy, vz, -(uz * vy)), cy = __builtin_fmaf(uz, vx, -(ux * vz)), cz = __builtin_fmaf(ux, vy, -(uy * vx));
    sx = sx + cx;
    sy = sy + cy;
    sz = sz + cz;
    twice_area = twice_area + sqrtf(__builtin_fmaf(cz, cz, __builtin_fmaf(cy, cy, cx * cx)));
  }
  const float len = sqrtf(__builtin_fmaf(sz, sz, __builtin_fmaf(sy, sy, sx * sx)));
  float4 n = make_float4(0.0f, 0.0f, 0.0f, twice_area / 6.0f);
  if (len > 0.0f) n.x = sx / len, n.y = sy / len, n.z = sz / len;
  reinterpret_cast<float4*>(normals)[i] = n;
}

extern "C" int mnerf_mesh_normals(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                  const int32_t* offsets, const int32_t* corners, float* normals, void* stream) {
  MNERF_REQUIRE(finish_sizes_ok(n_vertices, n_triangles), MNERF_E_RANGE, "mnerf_mesh_normals: %lld vertices / %lld triangles",
                (long long)n_vertices, (long long)n_triangles);
  if (n_vertices == 0) return MNERF_OK;
  MNERF_REQUIRE(vertices && offsets && normals, MNERF_E_NULL, "mnerf_mesh_normals: NULL vertices / offsets / normals");
  MNERF_REQUIRE(n_triangles == 0 || (triangles && corners), MNERF_E_NULL, "mnerf_mesh_normals: NULL triangles / corners");
  MNERF_REQUIRE(mnerf_aligned16(vertices) && mnerf_aligned16(normals), MNERF_E_ALIGN, "mnerf_mesh_normals: vertices / normals not 16B aligned");
  MNERF_REQUIRE(aligned_to(triangles, 4) && aligned_to(offsets, 4) && aligned_to(corners, 4), MNERF_E_ALIGN,
                "mnerf_mesh_normals: triangles / offsets / corners not 4B aligned");
  hipLaunchKernelGGL(normals_kernel, dim3(blocks_of(n_vertices)), dim3(PC_BLOCK), 0, (hipStream_t)stream, vertices, triangles, offsets,
                     corners, (int)n_vertices, normals);
  return mnerf_check_launch("mnerf_mesh_normals");
}
#pragma clang fp contract(fast)
