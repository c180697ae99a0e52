// Mesh finishing (include/mnerf.h "MESH FINISHING"): what turns the mesher's raw zero set - or any indexed triangle mesh in the
// project's layout - into a mesh one can use: the vertex -> corner adjacency, connected components and the removal of the small
// ones, Taubin smoothing of the positions, area-weighted vertex normals.
//
// Memory-bound streaming and gather kernels of one thread per vertex or per triangle, 256 threads per workgroup:
//   adj_zero / adj_count / the CSR offsets (scan.hip) / adj_fill / adj_sort_class
//                           corners per vertex, the two-level scan over them, the rows filled through a cursor, every row sorted
//                           by its own thread and classified
//   cc_init / cc_union / cc_flatten / cc_count / cc_largest / cc_keep
//                           a lock-free union-find over the triangles' edges, triangles per component, the keep bytes
//   compact_vcount / compact_tcount / the scan / compact_vertices / compact_triangles   the mesher's stable scan and scatter
//   smooth_step             one Jacobi step of the umbrella operator, ping-pong through the workspace
//   normals                 the corner sum of the triangles' cross products
//   dec_*                   decimation by quadric vertex clustering (section 6 below)
// THE DETERMINISM RULE: two runs give the same bytes in every output.  No floating-point atomic anywhere: every float sum runs over
// a CSR row in ascending corner order inside one thread.  Integer atomics only where the final memory contents do not depend on
// their order: the corner counts and triangle counts (add), the largest component (max), the union-find's hooks (whose final roots
// are the components' smallest rows whatever the order), and the row fill, which is sorted afterwards (the decimation's second
// table is not sorted: its rows are only searched for the existence of an entry).
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
  long long* head;   // int64 [2]: totals of the scans / the largest component
  int* per_vertex;   // int32 [V]   (adjacency, components, compact)
  ScanScratch sv, st;  // the scans over the vertices and over the triangles
  float* ping;       // fp32 [V][8], 16-byte aligned (smooth) - shares the bytes of the integer tables after the head
};
static FinishWorkspace finish_workspace(void* workspace, long long n_vertices, long long n_triangles) {
  FinishWorkspace w = {};
  if (n_vertices == 0) return w;
  Carve integers(workspace), floats(workspace);
  w.head = integers.array<long long>(2);
  w.per_vertex = integers.array<int>((size_t)n_vertices);
  w.sv = integers.scan(n_vertices);
  w.st = integers.scan(n_triangles);
  floats.array<long long>(2);
  w.ping = floats.array<float>(8 * (size_t)n_vertices, 16);
  w.bytes = integers.bytes() > floats.bytes() ? integers.bytes() : floats.bytes();
  return w;
}

static bool finish_sizes_ok(int64_t n_vertices, int64_t n_triangles) {
  return n_vertices >= 0 && n_triangles >= 0 && n_vertices <= FINISH_MAX_VERTICES && n_triangles <= FINISH_MAX_TRIANGLES;
}

extern "C" int64_t mnerf_mesh_finish_workspace_bytes(int64_t n_vertices, int64_t n_triangles) {
  if (!finish_sizes_ok(n_vertices, n_triangles)) return -1;
  return finish_workspace(nullptr, n_vertices, n_triangles).bytes;
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
  const FinishWorkspace w = finish_workspace(workspace, n_vertices, n_triangles);
  int* cursor = w.per_vertex;
  const int nv = (int)n_vertices;
  const long long n_corners = 3 * (long long)n_triangles;
  const dim3 threads(PC_BLOCK), vblocks(blocks_of(n_vertices)), cblocks(blocks_of(n_corners));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adj_zero_kernel, dim3(blocks_of(n_vertices + 1)), threads, 0, st, offsets, nv);
  if (n_corners) hipLaunchKernelGGL(adj_count_kernel, cblocks, threads, 0, st, triangles, n_corners, nv, offsets);
  csr_offsets_enqueue(offsets, nv, w.sv, w.head, cursor, st);
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
  const FinishWorkspace w = finish_workspace(workspace, n_vertices, n_triangles);
  int* largest = reinterpret_cast<int*>(w.head);
  int* tri_count = w.per_vertex;
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
  const long long row = scan_row(counts, tiles, before);
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
  const long long row = scan_row(counts, tiles, before);
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
  const FinishWorkspace w = finish_workspace(workspace, n_vertices, n_triangles);
  int* new_row = w.per_vertex;
  long long* count = reinterpret_cast<long long*>(counts);
  const int nv = (int)n_vertices;
  const long long nt = (long long)n_triangles;
  const dim3 threads(PC_BLOCK), vblocks(blocks_of(n_vertices)), tblocks(blocks_of(n_triangles));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(compact_vcount_kernel, vblocks, threads, 0, st, keep, nv, w.sv.counts);
  scan_enqueue(w.sv, count, st);
  hipLaunchKernelGGL(compact_vertices_kernel, vblocks, threads, 0, st, vertices, keep, nv, w.sv.counts, w.sv.tiles, new_row, vertices_out,
                     (long long)vertex_capacity);
  if (nt) hipLaunchKernelGGL(compact_tcount_kernel, tblocks, threads, 0, st, triangles, nt, nv, keep, w.st.counts);
  scan_enqueue(w.st, count + 1, st);  // (no triangle: the total, 0, alone)
  if (nt)
    hipLaunchKernelGGL(compact_triangles_kernel, tblocks, threads, 0, st, triangles, nt, nv, keep, new_row, w.st.counts, w.st.tiles,
                       triangles_out, (long long)triangle_capacity);
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
  float* ping = finish_workspace(workspace, n_vertices, n_triangles).ping;
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

// ------------------------------------------------------------------------------------------------ 6. decimation
// Quadric vertex clustering over a dense uniform grid (include/mnerf.h "mnerf_mesh_decimate"):
//   dec_cells / the CSR offsets / dec_fill        the cell of every vertex; the cell -> vertex rows, built as the adjacency's
//   dec_occupied / the scan / dec_representatives   the stable scan over the occupied cells; every cell's thread sorts its row,
//                           sums its quadric in fp64 and writes the new vertex
//   dec_candidates / adj_* / dec_first / the scan / dec_triangles   the new index triples, their adjacency, the first triangle
//                           of every set of three new rows, the stable scan and scatter over those
constexpr double MNERF_DECIMATE_REG = 1.0 / MNERF_DECIMATE_REG_INV;
struct DecGrid {
  float ox, oy, oz, cell;
  int gx, gy, gz;
};

__device__ __forceinline__ int dec_axis(float x, float origin, float cell, int g) {
  const float q = (x - origin) / cell;
  return (int)fmin(fmax((double)floorf(q), 0.0), (double)(g - 1));  // (clamped in double: q may be +-inf, g - 1 no fp32 number)
}

// the linear cell index of a position; -1: not finite
__device__ __forceinline__ int dec_cell_of(const float4 p, const DecGrid& g) {
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return -1;
  const int i = dec_axis(p.x, g.ox, g.cell, g.gx), j = dec_axis(p.y, g.oy, g.cell, g.gy), k = dec_axis(p.z, g.oz, g.cell, g.gz);
  return (k * g.gy + j) * g.gx + i;
}

__global__ __launch_bounds__(PC_BLOCK) void dec_cells_kernel(const float* __restrict__ vertices, int n_vertices, DecGrid g,
                                                             int* __restrict__ cell_of, int* __restrict__ cell_offsets) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const int c = dec_cell_of(reinterpret_cast<const float4*>(vertices)[(size_t)i * 2], g);
  cell_of[i] = c;
  if (c >= 0) atomicAdd(&cell_offsets[c], 1);
}

__global__ __launch_bounds__(PC_BLOCK) void dec_fill_kernel(const int* __restrict__ cell_of, int n_vertices, int* __restrict__ cursor,
                                                            int* __restrict__ members) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const int c = cell_of[i];
  if (c >= 0) members[atomicAdd(&cursor[c], 1)] = (int)i;  // (a slot of the cell's row: the row is sorted below)
}

__global__ __launch_bounds__(PC_BLOCK) void dec_occupied_kernel(const int* __restrict__ cell_offsets, int n_cells, int* __restrict__ counts) {
  const long long c = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  int total;
  block_prefix(c < n_cells && cell_offsets[c + 1] > cell_offsets[c], total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// ascending, in place, any length: a cell's row can be long and arrives in no order, so not the insertion sort of the short rows
__device__ __forceinline__ void dec_sort(int* a, int n) {
  for (int end = 1; end < n; ++end) {  // sift every element up into the max-heap a[0 .. end]
    int child = end;
    const int key = a[child];
    while (child > 0) {
      const int parent = (child - 1) >> 1;
      if (a[parent] >= key) break;
      a[child] = a[parent];
      child = parent;
    }
    a[child] = key;
  }
  for (int end = n - 1; end > 0; --end) {  // the largest to the end, the former last element sifted down from the root
    const int key = a[end];
    a[end] = a[0];
    int parent = 0;
    for (;;) {
      int child = 2 * parent + 1;
      if (child >= end) break;
      if (child + 1 < end && a[child + 1] > a[child]) ++child;
      if (a[child] <= key) break;
      a[parent] = a[child];
      parent = child;
    }
    a[parent] = key;
  }
}

__device__ __forceinline__ double dec_clamp(double x, double half) { return fmin(fmax(x, -half), half); }  // (a NaN -> -half)

__global__ __launch_bounds__(PC_BLOCK) void dec_representatives_kernel(
    const float* __restrict__ vertices, const int* __restrict__ triangles, const int* __restrict__ offsets, const int* __restrict__ corners,
    int n_vertices, int n_triangles, DecGrid g, int n_cells, const int* __restrict__ cell_offsets, int* __restrict__ members,
    const int* __restrict__ counts, const int* __restrict__ tiles, int* __restrict__ cell_row, float* __restrict__ out, long long capacity) {
  const long long c = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const int begin = c < n_cells ? cell_offsets[c] : 0, end = c < n_cells ? cell_offsets[c + 1] : 0;
  const bool occupied = end > begin;
  int total;
  const int before = block_prefix(occupied, total);
  if (c >= n_cells) return;
  const long long row = scan_row(counts, tiles, before);
  cell_row[c] = occupied ? (int)row : -1;
  if (!occupied || row >= capacity) return;
  dec_sort(members + begin, end - begin);
  const int plane = g.gx * g.gy, ck = (int)(c / plane), cj = (int)((c - (long long)ck * plane) / g.gx), ci = (int)(c - (long long)ck * plane - cj * g.gx);
  const double h = (double)g.cell;
  const double gx = (double)g.ox + ((double)ci + 0.5) * h, gy = (double)g.oy + ((double)cj + 0.5) * h, gz = (double)g.oz + ((double)ck + 0.5) * h;
  const float4* rows = reinterpret_cast<const float4*>(vertices);
  double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
  double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
  for (int m = begin; m < end; ++m) {
    const int v = members[m];
    const float4 p = rows[(size_t)v * 2], q = rows[(size_t)v * 2 + 1];
    sx = sx + ((double)p.x - gx), sy = sy + ((double)p.y - gy), sz = sz + ((double)p.z - gz);
    sw = sw + (double)p.w, sr = sr + (double)q.x, sg = sg + (double)q.y, sb = sb + (double)q.z;
    double vxx = 0.0, vxy = 0.0, vxz = 0.0, vyy = 0.0, vyz = 0.0, vzz = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
    for (int a = offsets[v]; a < offsets[v + 1]; ++a) {
      const int t = corners[a] / 3;
      int i0, i1, i2;
      if (!in_range(t, n_triangles) || !triangle_ok(triangles, t, n_vertices, i0, i1, i2)) continue;
      const float4 f0 = rows[(size_t)i0 * 2], f1 = rows[(size_t)i1 * 2], f2 = rows[(size_t)i2 * 2];
      if (!(isfinite(f0.x) && isfinite(f0.y) && isfinite(f0.z) && isfinite(f1.x) && isfinite(f1.y) && isfinite(f1.z) && isfinite(f2.x) &&
            isfinite(f2.y) && isfinite(f2.z)))
        continue;
      const double p0x = (double)f0.x - gx, p0y = (double)f0.y - gy, p0z = (double)f0.z - gz;
      const double ux = ((double)f1.x - gx) - p0x, uy = ((double)f1.y - gy) - p0y, uz = ((double)f1.z - gz) - p0z;
      const double tx = ((double)f2.x - gx) - p0x, ty = ((double)f2.y - gy) - p0y, tz = ((double)f2.z - gz) - p0z;
      const double nx = uy * tz - uz * ty, ny = uz * tx - ux * tz, nz = ux * ty - uy * tx;
      const double d = -((nx * p0x + ny * p0y) + nz * p0z);
      vxx = vxx + nx * nx, vxy = vxy + nx * ny, vxz = vxz + nx * nz, vyy = vyy + ny * ny, vyz = vyz + ny * nz, vzz = vzz + nz * nz;
      wx = wx + d * nx, wy = wy + d * ny, wz = wz + d * nz;
    }
    axx = axx + vxx, axy = axy + vxy, axz = axz + vxz, ayy = ayy + vyy, ayz = ayz + vyz, azz = azz + vzz;
    bx = bx + wx, by = by + wy, bz = bz + wz;
  }
  const double n = (double)(end - begin);
  const double mx = sx / n, my = sy / n, mz = sz / n;
  double x = mx, y = my, z = mz;
  const double lambda = MNERF_DECIMATE_REG * ((axx + ayy) + azz);
  if (lambda > 0.0) {  // (A + lambda I) x = lambda m - b by elimination without pivoting: symmetric positive definite, cond <= 1 / REG + 1
    const double m00 = axx + lambda, m11 = ayy + lambda, m22 = azz + lambda;
    const double r0 = lambda * mx - bx, r1 = lambda * my - by, r2 = lambda * mz - bz;
    const double l10 = axy / m00, l20 = axz / m00;
    const double e11 = m11 - l10 * axy, e12 = ayz - l10 * axz, e22 = m22 - l20 * axz;
    const double s1 = r1 - l10 * r0, s2 = r2 - l20 * r0;
    const double l21 = e12 / e11;
    z = (s2 - l21 * s1) / (e22 - l21 * e12);
    y = (s1 - e12 * z) / e11;
    x = ((r0 - axy * y) - axz * z) / m00;
  }
  const double half = 0.5 * h;
  float4* dst = reinterpret_cast<float4*>(out) + (size_t)row * 2;
  dst[0] = make_float4((float)(gx + dec_clamp(x, half)), (float)(gy + dec_clamp(y, half)), (float)(gz + dec_clamp(z, half)), (float)(sw / n));
  dst[1] = make_float4((float)(sr / n), (float)(sg / n), (float)(sb / n), 0.0f);
}

__global__ __launch_bounds__(PC_BLOCK) void dec_map_kernel(const int* __restrict__ cell_of, const int* __restrict__ cell_row, int n_vertices,
                                                           int* __restrict__ vertex_map) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const int c = cell_of[i];
  vertex_map[i] = c >= 0 ? cell_row[c] : -1;
}

// the new rows of every triangle; -1 -1 -1 unless it is a candidate
__global__ __launch_bounds__(PC_BLOCK) void dec_candidates_kernel(const int* __restrict__ triangles, long long n_triangles, int n_vertices,
                                                                  const int* __restrict__ cell_of, const int* __restrict__ cell_row,
                                                                  int* __restrict__ candidates) {
  const long long t = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (t >= n_triangles) return;
  int a, b, c, ra = -1, rb = -1, rc = -1;
  if (triangle_ok(triangles, t, n_vertices, a, b, c)) {
    const int ca = cell_of[a], cb = cell_of[b], cc = cell_of[c];
    if (ca >= 0 && cb >= 0 && cc >= 0 && ca != cb && cb != cc && ca != cc) ra = cell_row[ca], rb = cell_row[cb], rc = cell_row[cc];
  }
  candidates[3 * t] = ra, candidates[3 * t + 1] = rb, candidates[3 * t + 2] = rc;
}

__device__ __forceinline__ void dec_sort3(int& a, int& b, int& c) {
  int s;
  if (a > b) s = a, a = b, b = s;
  if (b > c) s = b, b = c, c = s;
  if (a > b) s = a, a = b, b = s;
}

// keep[t] = t is a candidate and no candidate before it has its three new rows: one thread per triangle walks the row of its smallest
// new vertex (in whatever order the fill left it: the answer is the existence of an earlier one)
__global__ __launch_bounds__(PC_BLOCK) void dec_first_kernel(const int* __restrict__ candidates, long long n_triangles,
                                                             const int* __restrict__ offsets, const int* __restrict__ corners,
                                                             unsigned char* __restrict__ keep, int* __restrict__ counts) {
  const long long t = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  bool first = false;
  if (t < n_triangles) {
    int a = candidates[3 * t], b = candidates[3 * t + 1], c = candidates[3 * t + 2];
    if (a >= 0) {
      dec_sort3(a, b, c);
      first = true;
      for (int k = offsets[a]; k < offsets[a + 1] && first; ++k) {
        const int u = corners[k] / 3;
        if (u >= t) continue;
        int d = candidates[3 * u], e = candidates[3 * u + 1], f = candidates[3 * u + 2];
        dec_sort3(d, e, f);
        first = !(d == a && e == b && f == c);
      }
    }
    keep[t] = first;
  }
  int total;
  block_prefix(first, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void dec_triangles_kernel(const int* __restrict__ candidates, long long n_triangles,
                                                                 const unsigned char* __restrict__ keep, const int* __restrict__ counts,
                                                                 const int* __restrict__ tiles, int* __restrict__ out, long long capacity) {
  const long long t = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const bool kept = t < n_triangles && keep[t];
  int total;
  const int before = block_prefix(kept, total);
  if (!kept) return;
  const long long row = scan_row(counts, tiles, before);
  if (row >= capacity) return;
  out[row * 3 + 0] = candidates[3 * t];
  out[row * 3 + 1] = candidates[3 * t + 1];
  out[row * 3 + 2] = candidates[3 * t + 2];
}

struct DecWorkspace {
  long long bytes;
  long long* head;                           // int64 [2]: the totals of the two CSR tables
  int *cell_of, *members;                    // int32 [V] the cell of a vertex | [V] the cells' rows
  int *cell_offsets, *cell_row;              // [N + 1] | [N] the fill cursor, then the cells' new rows
  ScanScratch sn;                            // the scans over the cells
  int* candidates;                           // [3 T]
  int *tri_offsets, *tri_cursor, *tri_corners;  // [V + 1] [V] [3 T] the candidates' adjacency and its cursor
  ScanScratch sv, st;                        // the scans over the vertices and over the triangles
  unsigned char* keep;                       // uint8 [T]
};
static DecWorkspace dec_workspace(void* workspace, long long n_vertices, long long n_triangles, long long n_cells) {
  DecWorkspace w = {};
  if (n_vertices == 0) return w;
  const size_t v = (size_t)n_vertices, t = (size_t)n_triangles, n = (size_t)n_cells;
  Carve c(workspace);
  w.head = c.array<long long>(2);
  w.cell_of = c.array<int>(v), w.members = c.array<int>(v);
  w.cell_offsets = c.array<int>(n + 1), w.cell_row = c.array<int>(n);
  w.sn = c.scan(n_cells);
  w.candidates = c.array<int>(3 * t);
  w.tri_offsets = c.array<int>(v + 1), w.tri_cursor = c.array<int>(v), w.tri_corners = c.array<int>(3 * t);
  w.sv = c.scan(n_vertices), w.st = c.scan(n_triangles);
  w.keep = c.array<unsigned char>(t);
  w.bytes = c.bytes();
  return w;
}

static bool dec_grid_ok(int32_t gx, int32_t gy, int32_t gz) {
  return gx >= 1 && gy >= 1 && gz >= 1 && (long long)gx * gy < (1ll << 31) && (long long)gx * gy * gz < (1ll << 31);
}

extern "C" int64_t mnerf_mesh_decimate_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int32_t gx, int32_t gy, int32_t gz) {
  if (!finish_sizes_ok(n_vertices, n_triangles) || !dec_grid_ok(gx, gy, gz)) return -1;
  return dec_workspace(nullptr, n_vertices, n_triangles, (long long)gx * gy * gz).bytes;
}

extern "C" int mnerf_mesh_decimate(const float* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_triangles,
                                   const int32_t* offsets, const int32_t* corners, float origin_x, float origin_y, float origin_z, float cell,
                                   int32_t gx, int32_t gy, int32_t gz, float* vertices_out, int64_t vertex_capacity, int32_t* triangles_out,
                                   int64_t triangle_capacity, int32_t* vertex_map, int64_t* counts, void* workspace, void* stream) {
  MNERF_REQUIRE(finish_sizes_ok(n_vertices, n_triangles), MNERF_E_RANGE, "mnerf_mesh_decimate: %lld vertices / %lld triangles",
                (long long)n_vertices, (long long)n_triangles);
  MNERF_REQUIRE(dec_grid_ok(gx, gy, gz), MNERF_E_RANGE, "mnerf_mesh_decimate: a grid of %d x %d x %d cells (every axis >= 1, the product < 2^31)",
                gx, gy, gz);
  MNERF_REQUIRE(std::isfinite(cell) && cell > 0.0f, MNERF_E_RANGE, "mnerf_mesh_decimate: cell=%g must be finite and > 0", (double)cell);
  MNERF_REQUIRE(std::isfinite(origin_x) && std::isfinite(origin_y) && std::isfinite(origin_z), MNERF_E_RANGE,
                "mnerf_mesh_decimate: origin (%g, %g, %g) is not finite", (double)origin_x, (double)origin_y, (double)origin_z);
  MNERF_REQUIRE(vertex_capacity >= 0 && triangle_capacity >= 0, MNERF_E_RANGE, "mnerf_mesh_decimate: capacities %lld / %lld",
                (long long)vertex_capacity, (long long)triangle_capacity);
  if (n_vertices == 0) return MNERF_OK;
  MNERF_REQUIRE(vertices && offsets && counts && workspace, MNERF_E_NULL, "mnerf_mesh_decimate: NULL vertices / offsets / counts / workspace");
  MNERF_REQUIRE(n_triangles == 0 || (triangles && corners), MNERF_E_NULL, "mnerf_mesh_decimate: NULL triangles / corners");
  MNERF_REQUIRE(vertex_capacity == 0 || vertices_out, MNERF_E_NULL, "mnerf_mesh_decimate: vertices_out is NULL");
  MNERF_REQUIRE(triangle_capacity == 0 || triangles_out, MNERF_E_NULL, "mnerf_mesh_decimate: triangles_out is NULL");
  MNERF_REQUIRE(mnerf_aligned16(vertices) && mnerf_aligned16(vertices_out) && mnerf_aligned16(workspace), MNERF_E_ALIGN,
                "mnerf_mesh_decimate: vertices / vertices_out / workspace not 16B aligned");
  MNERF_REQUIRE(aligned_to(triangles, 4) && aligned_to(offsets, 4) && aligned_to(corners, 4) && aligned_to(triangles_out, 4) &&
                    aligned_to(vertex_map, 4) && aligned_to(counts, 8),
                MNERF_E_ALIGN, "mnerf_mesh_decimate: triangles / offsets / corners / triangles_out / vertex_map / counts not aligned to 4 / 8 bytes");
  const long long n_cells_ll = (long long)gx * gy * gz;
  const DecWorkspace w = dec_workspace(workspace, n_vertices, n_triangles, n_cells_ll);
  long long* count = reinterpret_cast<long long*>(counts);
  const DecGrid g = {origin_x, origin_y, origin_z, cell, gx, gy, gz};
  const int nv = (int)n_vertices, nc = (int)n_cells_ll;
  const long long nt = (long long)n_triangles, n_corners = 3 * nt;
  const dim3 threads(PC_BLOCK), vblocks(blocks_of(n_vertices)), nblocks(blocks_of(n_cells_ll)), tblocks(blocks_of(nt)), cblocks(blocks_of(n_corners));
  hipStream_t st = (hipStream_t)stream;
  // the cell -> vertex rows
  hipLaunchKernelGGL(adj_zero_kernel, dim3(blocks_of(n_cells_ll + 1)), threads, 0, st, w.cell_offsets, nc);
  hipLaunchKernelGGL(dec_cells_kernel, vblocks, threads, 0, st, vertices, nv, g, w.cell_of, w.cell_offsets);
  csr_offsets_enqueue(w.cell_offsets, nc, w.sn, w.head, w.cell_row, st);
  hipLaunchKernelGGL(dec_fill_kernel, vblocks, threads, 0, st, w.cell_of, nv, w.cell_row, w.members);
  // the new vertices
  hipLaunchKernelGGL(dec_occupied_kernel, nblocks, threads, 0, st, w.cell_offsets, nc, w.sn.counts);
  scan_enqueue(w.sn, count, st);
  hipLaunchKernelGGL(dec_representatives_kernel, nblocks, threads, 0, st, vertices, triangles, offsets, corners, nv, (int)nt, g, nc,
                     w.cell_offsets, w.members, w.sn.counts, w.sn.tiles, w.cell_row, vertices_out, (long long)vertex_capacity);
  if (vertex_map) hipLaunchKernelGGL(dec_map_kernel, vblocks, threads, 0, st, w.cell_of, w.cell_row, nv, vertex_map);
  // the new triangles: the adjacency of the candidates over the new rows (at most V of them), the first of every set, the scatter
  if (nt) {
    hipLaunchKernelGGL(dec_candidates_kernel, tblocks, threads, 0, st, triangles, nt, nv, w.cell_of, w.cell_row, w.candidates);
    hipLaunchKernelGGL(adj_zero_kernel, dim3(blocks_of(n_vertices + 1)), threads, 0, st, w.tri_offsets, nv);
    hipLaunchKernelGGL(adj_count_kernel, cblocks, threads, 0, st, w.candidates, n_corners, nv, w.tri_offsets);
    csr_offsets_enqueue(w.tri_offsets, nv, w.sv, w.head + 1, w.tri_cursor, st);
    hipLaunchKernelGGL(adj_fill_kernel, cblocks, threads, 0, st, w.candidates, n_corners, nv, w.tri_cursor, w.tri_corners);
    hipLaunchKernelGGL(dec_first_kernel, tblocks, threads, 0, st, w.candidates, nt, w.tri_offsets, w.tri_corners, w.keep, w.st.counts);
  }
  scan_enqueue(w.st, count + 1, st);  // (no triangle: the total, 0, alone)
  if (nt)
    hipLaunchKernelGGL(dec_triangles_kernel, tblocks, threads, 0, st, w.candidates, nt, w.keep, w.st.counts, w.st.tiles, triangles_out,
                       (long long)triangle_capacity);
  return mnerf_check_launch("mnerf_mesh_decimate");
}
#pragma clang fp contract(fast)
