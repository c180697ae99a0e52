// What the geometry-export kernels share (fusion.hip: consistency, point cloud; mesh.hip: TSDF volume, mesher): the camera with its
// host-inverted matrices, the fp32 projection chain, the value of a depth texel, and the integer workgroup scans of the stable
// compactions.  Include after common.hpp, under `#pragma clang fp contract(off)`: every operation rounds on its own and the FMAs
// are the explicit ones of the helpers.
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
