// Evaluation on the device (gfx950): PSNR and SSIM of rendered frames against their ground truth, one row of four doubles per image.
//
// Replaces (paths relative to the reference):
//   misc/metrics.py:19-33    set_inputs: the DTU mask (masked pixels zeroed in both images) or the 80 % centre crop
//   misc/metrics.py:36-45    PSNR over the kept pixels; structural_similarity(channel_axis=-1): 7x7 uniform window, sample
//                            covariance, K1 = 0.01, K2 = 0.03, data_range = 2 (float images without a data_range)
//   coach.py:316-453         the per-image .cpu().numpy() + five scipy.ndimage.uniform_filter passes per channel
//
// A workgroup owns a tile of MET_TH x MET_TW windows of one image (blockIdx.y).  It stages the tile plus the 6-pixel halo of both
// images in LDS - pred is read channel-last, gt channel-first, both along their contiguous axis -, applying the mask or the crop
// on the way; then, channel by channel, it forms the 7-tap row sums of the five moments x, y, xx, yy, xy and from those the 7-tap
// column sums, evaluates the SSIM expression of every window, and adds up its windows' values, the squared errors of the pixels it
// owns and their count.  Inputs are fp32; every product and every sum is fp64 (the variance is a difference of two nearly equal
// numbers set against C2 = 3.6e-3: fp32 moments miss by 1e-5 on flat, bright images).
//
// Reductions are deterministic (the rule of optim.hip): a workgroup reduces in a fixed shuffle / LDS order into its own three
// workspace slots, a second kernel adds the slots of an image in a fixed order.  No floating-point atomics; an image's numbers
// depend neither on the other images of the batch nor on n_images.
#include "common.hpp"

namespace {

constexpr int MET_THREADS = 256;
constexpr int MET_WIN = 7;
constexpr int MET_HALO = MET_WIN - 1;
constexpr int MET_TH = 16, MET_TW = 32;                        // windows of one tile
constexpr int MET_SH = MET_TH + MET_HALO, MET_SW = MET_TW + MET_HALO;  // staged pixels of one tile
constexpr int MET_SLOTS = 3;                                   // per tile: sum of SSIM values, sum of squared errors, kept pixels
// LDS: 2 x 3 x 22 x 38 floats (20 064 B) + 5 x 22 x 32 doubles (28 160 B) + 22 x 38 flags: 49 KiB, three workgroups per CU

struct MetShape {
  int32_t height, width;    // the images as stored
  int32_t y0, x0;           // origin of the processed image inside them (the crop; 0 with a mask)
  int32_t ph, pw;           // the processed image
  int32_t tiles_y, tiles_x;
};

__host__ __device__ inline int met_tiles(int pixels, int tile) { return (pixels - MET_HALO + tile - 1) / tile; }

// fixed-order sums of three values over the workgroup; valid in thread 0
__device__ __forceinline__ void met_block_sum3(double& a, double& b, double& c, double (*red)[MET_SLOTS]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
    c += __shfl_xor(c, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = a;
    red[threadIdx.x >> 6][1] = b;
    red[threadIdx.x >> 6][2] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0][0], b = red[0][1], c = red[0][2];
#pragma unroll
    for (int i = 1; i < MET_THREADS / 64; ++i) a += red[i][0], b += red[i][1], c += red[i][2];
  }
}

__global__ __launch_bounds__(MET_THREADS) void image_metrics_tile_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                         int64_t gt_image_stride,
                                                                         const uint8_t* __restrict__ invalid_mask, MetShape s,
                                                                         double* __restrict__ slots) {
  __shared__ float sp[3][MET_SH][MET_SW];
  __shared__ float sg[3][MET_SH][MET_SW];
  __shared__ uint8_t keep[MET_SH][MET_SW];
  __shared__ double rs[5][MET_SH][MET_TW];
  __shared__ double red[MET_THREADS / 64][MET_SLOTS];

  const int tid = (int)threadIdx.x;
  const int img = (int)blockIdx.y;
  const int ty = (int)blockIdx.x / s.tiles_x, tx = (int)blockIdx.x % s.tiles_x;
  const int py0 = ty * MET_TH, px0 = tx * MET_TW;  // the tile's first pixel = its first window, in the processed image
  const int64_t plane = (int64_t)s.height * s.width;
  const float* pimg = pred + (int64_t)img * plane * 3;
  const float* gimg = gt + (int64_t)img * gt_image_stride;
  const uint8_t* mimg = invalid_mask ? invalid_mask + (int64_t)img * plane : nullptr;

  // ---- stage: pixels outside the processed image and masked pixels are 0 in both images
  for (int i = tid; i < MET_SH * MET_SW; i += MET_THREADS) {
    const int r = i / MET_SW, c = i % MET_SW;
    const int py = py0 + r, px = px0 + c;
    bool k = py < s.ph && px < s.pw;
    if (k && mimg) k = mimg[(int64_t)(py + s.y0) * s.width + (px + s.x0)] == 0;
    keep[r][c] = k ? 1 : 0;
  }
  __syncthreads();
  for (int i = tid; i < MET_SH * MET_SW * 3; i += MET_THREADS) {  // pred: a staged row is 3 * MET_SW consecutive floats
    const int r = i / (MET_SW * 3), j = i % (MET_SW * 3);
    const int c = j / 3, ch = j % 3;
    float v = 0.0f;
    if (keep[r][c]) v = pimg[((int64_t)(py0 + r + s.y0) * s.width + (px0 + c + s.x0)) * 3 + ch];
    sp[ch][r][c] = v;
  }
  for (int i = tid; i < 3 * MET_SH * MET_SW; i += MET_THREADS) {  // gt: a staged row of one channel is MET_SW consecutive floats
    const int ch = i / (MET_SH * MET_SW), j = i % (MET_SH * MET_SW);
    const int r = j / MET_SW, c = j % MET_SW;
    float v = 0.0f;
    if (keep[r][c]) v = gimg[(int64_t)ch * plane + (int64_t)(py0 + r + s.y0) * s.width + (px0 + c + s.x0)];
    sg[ch][r][c] = v;
  }
  __syncthreads();

  // ---- squared errors of the pixels this tile owns: its MET_TH x MET_TW pixels, and the halo behind the last tile of a direction
  double se = 0.0, cnt = 0.0;
  const int own_h = ty == s.tiles_y - 1 ? MET_SH : MET_TH, own_w = tx == s.tiles_x - 1 ? MET_SW : MET_TW;
  for (int i = tid; i < MET_SH * MET_SW; i += MET_THREADS) {
    const int r = i / MET_SW, c = i % MET_SW;
    if (r < own_h && c < own_w && keep[r][c]) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double d = (double)sp[ch][r][c] - (double)sg[ch][r][c];
        se += d * d;
      }
      cnt += 1.0;
    }
  }

  // ---- SSIM, channel by channel
  const int nwy = min(MET_TH, s.ph - MET_HALO - py0), nwx = min(MET_TW, s.pw - MET_HALO - px0);  // this tile's windows
  const double c1 = (0.01 * 2.0) * (0.01 * 2.0), c2 = (0.03 * 2.0) * (0.03 * 2.0);
  const double inv_n = 1.0 / (double)(MET_WIN * MET_WIN), cov_norm = (double)(MET_WIN * MET_WIN) / (double)(MET_WIN * MET_WIN - 1);
  double ss = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    for (int i = tid; i < MET_SH * MET_TW; i += MET_THREADS) {  // 7-tap row sums
      const int r = i / MET_TW, c = i % MET_TW;
      double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
      for (int t = 0; t < MET_WIN; ++t) {
        const double x = (double)sp[ch][r][c + t], y = (double)sg[ch][r][c + t];
        mx += x, my += y, mxx += x * x, myy += y * y, mxy += x * y;
      }
      rs[0][r][c] = mx, rs[1][r][c] = my, rs[2][r][c] = mxx, rs[3][r][c] = myy, rs[4][r][c] = mxy;
    }
    __syncthreads();
    for (int i = tid; i < MET_TH * MET_TW; i += MET_THREADS) {  // 7-tap column sums of the row sums, one window each
      const int r = i / MET_TW, c = i % MET_TW;
      if (r < nwy && c < nwx) {
        double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
        for (int t = 0; t < MET_WIN; ++t) {
          mx += rs[0][r + t][c], my += rs[1][r + t][c], mxx += rs[2][r + t][c], myy += rs[3][r + t][c], mxy += rs[4][r + t][c];
        }
        const double ux = mx * inv_n, uy = my * inv_n;
        const double vx = cov_norm * (mxx * inv_n - ux * ux), vy = cov_norm * (myy * inv_n - uy * uy);
        const double vxy = cov_norm * (mxy * inv_n - ux * uy);
        ss += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
      }
    }
    __syncthreads();
  }

  met_block_sum3(ss, se, cnt, red);
  if (tid == 0) {
    double* out = slots + ((int64_t)img * gridDim.x + blockIdx.x) * MET_SLOTS;
    out[0] = ss, out[1] = se, out[2] = cnt;
  }
}

// one workgroup per image adds that image's slots in a fixed order and writes PSNR dB, SSIM, MSE, kept pixels
__global__ __launch_bounds__(MET_THREADS) void image_metrics_final_kernel(const double* __restrict__ slots, int n_tiles,
                                                                          double n_windows, double* __restrict__ out) {
  __shared__ double red[MET_SLOTS][MET_THREADS];
  const int tid = (int)threadIdx.x;
  const double* mine = slots + (int64_t)blockIdx.x * n_tiles * MET_SLOTS;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int j = tid; j < n_tiles; j += MET_THREADS) a += mine[j * MET_SLOTS], b += mine[j * MET_SLOTS + 1], c += mine[j * MET_SLOTS + 2];
  red[0][tid] = a, red[1][tid] = b, red[2][tid] = c;
  __syncthreads();
#pragma unroll
  for (int off = MET_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[0][tid] += red[0][tid + off], red[1][tid] += red[1][tid + off], red[2][tid] += red[2][tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    const double kept = red[2][0];
    const double mse = red[1][0] / (3.0 * kept);  // no kept pixel: 0 / 0 = NaN, as numpy's mean of nothing
    double* o = out + (int64_t)blockIdx.x * 4;
    o[0] = -10.0 * log(mse) / log(10.0);          // mse = 0: +inf
    o[1] = red[0][0] / (3.0 * n_windows);
    o[2] = mse;
    o[3] = kept;
  }
}

// the processed image and its tiling; false below the limits (7 with a mask: one window; 10 without: the crop is 8 x 8)
bool met_shape(int32_t height, int32_t width, bool masked, MetShape* s) {
  const int32_t least = masked ? MET_WIN : 10;
  if (height < least || width < least) return false;
  s->height = height, s->width = width;
  s->y0 = masked ? 0 : height / 10, s->x0 = masked ? 0 : width / 10;
  s->ph = height - 2 * s->y0, s->pw = width - 2 * s->x0;
  s->tiles_y = met_tiles(s->ph, MET_TH), s->tiles_x = met_tiles(s->pw, MET_TW);
  return true;
}

}  // namespace

extern "C" int64_t mnerf_image_metrics_workspace_bytes(int32_t n_images, int32_t height, int32_t width) {
  MetShape s;  // the whole image has at least as many tiles as its crop
  if (n_images < 1 || !met_shape(height, width, true, &s)) return -1;
  return (int64_t)n_images * s.tiles_y * s.tiles_x * MET_SLOTS * (int64_t)sizeof(double);
}

extern "C" int mnerf_image_metrics(const float* pred, const float* gt, int64_t gt_image_stride, const uint8_t* invalid_mask,
                                   int32_t n_images, int32_t height, int32_t width, void* workspace, double* out, void* stream) {
  MNERF_REQUIRE(pred && gt && workspace && out, MNERF_E_NULL, "mnerf_image_metrics: pred / gt / workspace / out is NULL");
  MNERF_REQUIRE(n_images >= 1 && n_images <= 65535, MNERF_E_RANGE, "mnerf_image_metrics: n_images %d outside [1, 65535]", n_images);
  MetShape s;
  MNERF_REQUIRE(met_shape(height, width, invalid_mask != nullptr, &s), MNERF_E_RANGE,
                "mnerf_image_metrics: %d x %d image, the smallest is %s", height, width,
                invalid_mask ? "7 x 7 with a mask (one window)" : "10 x 10 without a mask (an 8 x 8 crop)");
  MNERF_REQUIRE((int64_t)height * width <= INT32_MAX / 3, MNERF_E_RANGE, "mnerf_image_metrics: %d x %d image is too large", height, width);
  MNERF_REQUIRE(gt_image_stride >= (int64_t)3 * height * width, MNERF_E_RANGE,
                "mnerf_image_metrics: gt_image_stride %lld is less than one image (%lld floats)", (long long)gt_image_stride,
                (long long)3 * height * width);
  MNERF_REQUIRE((((uintptr_t)workspace) & 7u) == 0 && (((uintptr_t)out) & 7u) == 0, MNERF_E_ALIGN,
                "mnerf_image_metrics: workspace / out must be 8-byte aligned");
  const int n_tiles = s.tiles_y * s.tiles_x;
  hipStream_t st = (hipStream_t)stream;
  image_metrics_tile_kernel<<<dim3(n_tiles, n_images), dim3(MET_THREADS), 0, st>>>(pred, gt, gt_image_stride, invalid_mask, s,
                                                                                     (double*)workspace);
  if (int rc = mnerf_check_launch("mnerf_image_metrics (tiles)")) return rc;
  const double n_windows = (double)(s.ph - MET_HALO) * (double)(s.pw - MET_HALO);
  image_metrics_final_kernel<<<dim3(n_images), dim3(MET_THREADS), 0, st>>>((const double*)workspace, n_tiles, n_windows, out);
  return mnerf_check_launch("mnerf_image_metrics");
}
