// The two-level integer scan behind every stable compaction and every CSR table of the geometry export (fusion.hip, mesh.hip,
// mesh_finish.hip; the contract is stated at the declarations in fusion_common.hpp).  One definition of each kernel, and the only
// place that enqueues them.
#include "common.hpp"

#pragma clang fp contract(off)

#include "fusion_common.hpp"

// values[n], one per thread -> the workgroups' sums
__global__ __launch_bounds__(PC_BLOCK) void scan_blocksum_kernel(const int* __restrict__ values, int n, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const int v[4] = {i < n ? values[i] : 0, 0, 0, 0};
  int total;
  tile_scan(v, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one workgroup per tile of PC_TILE counts: every count -> its exclusive prefix inside the tile, tiles[tile] = the tile's sum
__global__ __launch_bounds__(PC_BLOCK) void scan_tiles_kernel(int* __restrict__ counts, int n_blocks, int* __restrict__ tiles) {
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

// One workgroup: the exclusive scan of the tiles' sums in rounds of PC_TILE with a carried sum, and the grand total.  NO TEST
// REACHES THE SECOND ROUND: it takes more than 1024 tiles, that is 2^28 elements; the carry is correct by inspection only.
__global__ __launch_bounds__(PC_BLOCK) void scan_total_kernel(int* __restrict__ tiles, int n_tiles, long long* __restrict__ count) {
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

// offsets[i]: the count -> the exclusive prefix; cursor[i] = the same; offsets[n] = the total
__global__ __launch_bounds__(PC_BLOCK) void csr_offsets_kernel(int* __restrict__ offsets, int n, const int* __restrict__ counts,
                                                               const int* __restrict__ tiles, int* __restrict__ cursor) {
  const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
  const int mine = i < n ? offsets[i] : 0;
  const int v[4] = {mine, 0, 0, 0};
  int total;
  const int before = tile_scan(v, total);
  if (i >= n) return;
  const int first = (int)scan_row(counts, tiles, before);
  offsets[i] = first;
  cursor[i] = first;
  if (i == n - 1) offsets[n] = first + mine;
}

void scan_enqueue(const ScanScratch& s, long long* total, hipStream_t st) {
  if (s.n_tiles) hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)s.n_tiles), dim3(PC_BLOCK), 0, st, s.counts, (int)s.blocks, s.tiles);
  hipLaunchKernelGGL(scan_total_kernel, dim3(1), dim3(PC_BLOCK), 0, st, s.tiles, (int)s.n_tiles, total);
}

void scan_values_enqueue(const int* values, int n, const ScanScratch& s, long long* total, hipStream_t st) {
  if (s.blocks) hipLaunchKernelGGL(scan_blocksum_kernel, dim3((unsigned)s.blocks), dim3(PC_BLOCK), 0, st, values, n, s.counts);
  scan_enqueue(s, total, st);
}

void csr_offsets_enqueue(int* offsets, int n, const ScanScratch& s, long long* total, int* cursor, hipStream_t st) {
  scan_values_enqueue(offsets, n, s, total, st);
  if (s.blocks) hipLaunchKernelGGL(csr_offsets_kernel, dim3((unsigned)s.blocks), dim3(PC_BLOCK), 0, st, offsets, n, s.counts, s.tiles, cursor);
}
#pragma clang fp contract(fast)
