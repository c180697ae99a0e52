// LPIPS (VGG-16 variant of lpips v0.1) on the device (gfx950): one double per test image, no frame leaves the device.
//
// Replaces (paths relative to the reference):
//   misc/metrics.py:14-17,47-52   lpips.LPIPS(net='vgg') on the masked / cropped frames, one host round trip per image
//   misc/metrics.py:19-33         set_inputs: the DTU mask (masked pixels zeroed in both images) or the 80 % centre crop
// and, in this project, matchnerf_amd/metrics.py: LPIPSVGG evaluated with library convolutions behind EvalTools.
//
// The 13 convolutions are mnerf_conv2d (conv.hip: three-product split-fp16 on v_mfma_f32_32x32x16_f16, bias, ReLU as leaky_slope 0,
// absmax hand-off; 256 / 512 output channels as blocks of 128 along grid.y).  This file adds what a VGG pass needs around them:
//   lpips_input_kernel    mask or crop, 2x - 1, (x - shift) / scale of the 2n images, written as the 32-channel NCHW tensor the first
//                         convolution reads (channels 3..31 zero: its weights there are zero as well), the pair's largest magnitude
//                         into the pair's absmax region
//   maxpool2x2_kernel     F.max_pool2d(x, 2, 2): floor sizes, NCHW
//   lpips_head_kernel     one stage of the distance of a pair: channel norms, unit(a) - unit(b), squares weighted by the stage's head,
//                         summed over channels and the workgroup's 64 pixels, times 1 / (h w) - all fp64 - into the workgroup's slot
//   lpips_sum_kernel      one workgroup per image adds the image's slots (all stages) in a fixed order
// mnerf_lpips_vgg walks the network ONE PAIR (pred i, gt i) at a time: the gain of every operand tensor comes from the pair's own
// absmax regions, so the number of image i does not depend on the other images of the batch, and pred == gt gives exactly 0 (both
// images of a pair go through the same instructions with the same gain, and the head's difference is not contracted into an FMA).
// Reductions are deterministic (the rule of metrics.hip): no floating-point atomics.
#include "common.hpp"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_LAYERS = 13, LP_STAGES = 5;
constexpr int LP_C0 = 32;                       // channels of the stored network input (3 real ones)
constexpr int LP_HEAD_PIX = 64;                 // pixels of one head workgroup (4 waves = 4 channel groups)
const int LP_CIN[LP_LAYERS] = {LP_C0, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int LP_COUT[LP_LAYERS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int LP_STAGE_END[LP_STAGES] = {1, 3, 6, 9, 12};  // the layer whose output is the stage's feature map
const int LP_STAGE_C[LP_STAGES] = {64, 128, 256, 512, 512};

struct LpShape {
  int32_t height, width;  // the frames as stored
  int32_t y0, x0;         // origin of the processed image inside them (the crop; 0 with a mask)
  int32_t ph, pw;         // the processed image = the network's input size
};

// the processed image; false below 16 x 16 (four 2x2 pools: the last stage would be empty)
bool lp_shape(int32_t height, int32_t width, bool masked, LpShape* s) {
  if (height < 1 || width < 1) return false;
  s->height = height, s->width = width;
  s->y0 = masked ? 0 : height / 10, s->x0 = masked ? 0 : width / 10;
  s->ph = height - 2 * s->y0, s->pw = width - 2 * s->x0;
  return s->ph >= 16 && s->pw >= 16;
}

inline int64_t lp_align(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
inline int64_t lp_head_slots(int h, int w) { return ((int64_t)h * w + LP_HEAD_PIX - 1) / LP_HEAD_PIX; }
int64_t lp_image_slots(const LpShape& s) {
  int64_t n = 0;
  for (int l = 0; l < LP_STAGES; ++l) n += lp_head_slots(s.ph >> l, s.pw >> l);
  return n;
}
// workspace: [activation A | activation B] shared by all pairs, then per image [network input | 14 absmax regions | head slots]
struct LpLayout {
  int64_t act_bytes, in_bytes, absmax_bytes, slot_bytes, per_image, total;
};
LpLayout lp_layout(const LpShape& s, int n_images) {
  LpLayout L;
  const int64_t hw = (int64_t)s.ph * s.pw;
  L.act_bytes = lp_align(2 * 64 * hw * 4);  // the largest activation of a pair: 64 channels at full size
  L.in_bytes = lp_align(2 * LP_C0 * hw * 4);
  L.absmax_bytes = (int64_t)(LP_LAYERS + 1) * MNERF_ABSMAX_FLOATS * 4;
  L.slot_bytes = lp_align(lp_image_slots(s) * 8);
  L.per_image = L.in_bytes + L.absmax_bytes + L.slot_bytes;
  L.total = 2 * L.act_bytes + (int64_t)n_images * L.per_image;
  return L;
}

__device__ __forceinline__ float lp_net_input(float v, float shift, float scale) {
  return (__builtin_fmaf(2.0f, v, -1.0f) - shift) / scale;  // 2x - 1 is exact in one rounding; LPIPSVGG's ScalingLayer
}

__global__ __launch_bounds__(LP_THREADS) void lpips_input_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                int64_t gt_image_stride, const uint8_t* __restrict__ invalid_mask,
                                                                LpShape s, float* __restrict__ ws_images, int64_t per_image_floats,
                                                                int64_t absmax_offset_floats) {
  __shared__ float red[LP_THREADS / 64];
  const int img = (int)blockIdx.y;
  const int64_t plane = (int64_t)s.height * s.width, hw = (int64_t)s.ph * s.pw;
  float* out = ws_images + (int64_t)img * per_image_floats;  // [2][LP_C0][ph][pw]: pred, gt
  const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
  float m = 0.0f;
  if (i < hw) {
    const int py = (int)(i / s.pw), px = (int)(i - (int64_t)py * s.pw);
    const int64_t src = (int64_t)(py + s.y0) * s.width + (px + s.x0);
    const bool keep = !invalid_mask || invalid_mask[(int64_t)img * plane + src] == 0;
    const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float p = keep ? pred[((int64_t)img * plane + src) * 3 + c] : 0.0f;  // zeroed in [0, 1] space
      const float g = keep ? gt[(int64_t)img * gt_image_stride + (int64_t)c * plane + src] : 0.0f;
      const float vp = lp_net_input(p, shift[c], scale[c]), vg = lp_net_input(g, shift[c], scale[c]);
      out[(int64_t)c * hw + i] = vp;
      out[(int64_t)(LP_C0 + c) * hw + i] = vg;
      m = fmaxf(m, fmaxf(fabsf(vp), fabsf(vg)));
    }
    for (int c = 3; c < LP_C0; ++c) {
      out[(int64_t)c * hw + i] = 0.0f;
      out[(int64_t)(LP_C0 + c) * hw + i] = 0.0f;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    mnerf_absmax_merge(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), out + absmax_offset_floats);
}

__global__ __launch_bounds__(LP_THREADS) void maxpool2x2_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t planes,
                                                               int h, int w) {
  const int ho = h >> 1, wo = w >> 1;
  const int64_t total = planes * ho * wo;
  const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t pl = i / ((int64_t)ho * wo);
  const int rem = (int)(i - pl * ho * wo);
  const int oy = rem / wo, ox = rem - oy * wo;
  const float* p = in + pl * h * w + (int64_t)(2 * oy) * w + 2 * ox;
  out[i] = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[w], p[w + 1]));
}

// unit(a) - unit(b) must be exactly 0 for a == b: no FMA contraction of the difference
#pragma clang fp contract(off)
__global__ __launch_bounds__(LP_THREADS) void lpips_head_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                               const float* __restrict__ head_w, int c, int hw, double inv_hw,
                                                               double* __restrict__ slots) {
  __shared__ double red[LP_THREADS / 64][LP_HEAD_PIX][2];
  const int px = (int)threadIdx.x & 63, cg = (int)threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * LP_HEAD_PIX + px;
  const bool live = p < hw;
  const int64_t pc = live ? p : hw - 1;
  double sa = 0.0, sb = 0.0;
  for (int ch = cg; ch < c; ch += LP_THREADS / 64) {
    const double x = (double)a[(int64_t)ch * hw + pc], y = (double)b[(int64_t)ch * hw + pc];
    sa += x * x;
    sb += y * y;
  }
  red[cg][px][0] = sa, red[cg][px][1] = sb;
  __syncthreads();
  const double na = sqrt(((red[0][px][0] + red[1][px][0]) + red[2][px][0]) + red[3][px][0]) + 1e-10;
  const double nb = sqrt(((red[0][px][1] + red[1][px][1]) + red[2][px][1]) + red[3][px][1]) + 1e-10;
  const double ia = 1.0 / na, ib = 1.0 / nb;
  double acc = 0.0;
  for (int ch = cg; ch < c; ch += LP_THREADS / 64) {
    const double x = (double)a[(int64_t)ch * hw + pc], y = (double)b[(int64_t)ch * hw + pc];
    const double d = x * ia - y * ib;
    acc += (double)head_w[ch] * (d * d);
  }
  __syncthreads();
  red[cg][px][0] = live ? acc : 0.0;
  __syncthreads();
  if (cg == 0) {  // wave 0: the four channel groups of its pixel, then the 64 pixels, in a fixed order
    double t = ((red[0][px][0] + red[1][px][0]) + red[2][px][0]) + red[3][px][0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (px == 0) slots[blockIdx.x] = t * inv_hw;
  }
}
#pragma clang fp contract(fast)

__global__ __launch_bounds__(LP_THREADS) void lpips_sum_kernel(const double* __restrict__ slots, int64_t image_stride_doubles,
                                                              int n_slots, double* __restrict__ out) {
  __shared__ double red[LP_THREADS];
  const int tid = (int)threadIdx.x;
  const double* mine = slots + (int64_t)blockIdx.x * image_stride_doubles;
  double a = 0.0;
  for (int j = tid; j < n_slots; j += LP_THREADS) a += mine[j];
  red[tid] = a;
  __syncthreads();
#pragma unroll
  for (int off = LP_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = red[0];
}

int lp_maxpool(const float* in, float* out, int64_t planes, int h, int w, hipStream_t st) {
  const int64_t total = planes * (h >> 1) * (w >> 1);
  if (total == 0) return MNERF_OK;
  maxpool2x2_kernel<<<dim3((unsigned)((total + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, st>>>(in, out, planes, h, w);
  return mnerf_check_launch("mnerf_maxpool2x2");
}

int lp_head(const float* a, const float* b, const float* head_w, int c, int h, int w, double* slots, hipStream_t st) {
  const int hw = h * w;
  lpips_head_kernel<<<dim3((unsigned)lp_head_slots(h, w)), dim3(LP_THREADS), 0, st>>>(a, b, head_w, c, hw, 1.0 / (double)hw, slots);
  return mnerf_check_launch("mnerf_lpips_head");
}

}  // namespace

extern "C" int64_t mnerf_lpips_wstream_floats(int32_t layer) {
  if (layer < 0 || layer >= LP_LAYERS) return 0;
  return mnerf_conv_wstream_floats(LP_CIN[layer], LP_COUT[layer], 3);
}

extern "C" int64_t mnerf_lpips_workspace_bytes(int32_t n_images, int32_t height, int32_t width, int32_t masked) {
  LpShape s;
  if (n_images < 1 || !lp_shape(height, width, masked != 0, &s)) return -1;
  return lp_layout(s, n_images).total;
}

extern "C" int mnerf_maxpool2x2(const float* in, float* out, int64_t planes, int32_t h, int32_t w, void* stream) {
  MNERF_REQUIRE(planes >= 0 && h >= 1 && w >= 1, MNERF_E_RANGE, "mnerf_maxpool2x2: planes=%lld h=%d w=%d", (long long)planes, h, w);
  MNERF_REQUIRE(planes * (h >> 1) * (w >> 1) <= (int64_t)INT32_MAX * LP_THREADS, MNERF_E_RANGE, "mnerf_maxpool2x2: too many elements");
  if (planes == 0 || h < 2 || w < 2) return MNERF_OK;
  MNERF_REQUIRE(in && out, MNERF_E_NULL, "mnerf_maxpool2x2: in / out is NULL");
  return lp_maxpool(in, out, planes, h, w, (hipStream_t)stream);
}

extern "C" int64_t mnerf_lpips_head_slots(int32_t h, int32_t w) { return (h < 1 || w < 1) ? -1 : lp_head_slots(h, w); }

extern "C" int mnerf_lpips_head(const float* feat_a, const float* feat_b, const float* head_w, int32_t channels, int32_t h, int32_t w,
                                double* slots, void* stream) {
  MNERF_REQUIRE(feat_a && feat_b && head_w && slots, MNERF_E_NULL, "mnerf_lpips_head: feat_a / feat_b / head_w / slots is NULL");
  MNERF_REQUIRE(channels >= 1 && h >= 1 && w >= 1 && (int64_t)channels * h * w <= INT32_MAX, MNERF_E_RANGE,
                "mnerf_lpips_head: channels=%d h=%d w=%d", channels, h, w);
  MNERF_REQUIRE((((uintptr_t)slots) & 7u) == 0, MNERF_E_ALIGN, "mnerf_lpips_head: slots must be 8-byte aligned");
  return lp_head(feat_a, feat_b, head_w, channels, h, w, slots, (hipStream_t)stream);
}

extern "C" int mnerf_lpips_sum(const double* slots, int64_t image_stride, int32_t n_slots, int32_t n_images, double* out, void* stream) {
  MNERF_REQUIRE(slots && out, MNERF_E_NULL, "mnerf_lpips_sum: slots / out is NULL");
  MNERF_REQUIRE(n_slots >= 1 && n_images >= 1 && image_stride >= n_slots, MNERF_E_RANGE, "mnerf_lpips_sum: n_slots=%d n_images=%d stride=%lld",
                n_slots, n_images, (long long)image_stride);
  MNERF_REQUIRE((((uintptr_t)slots) & 7u) == 0 && (((uintptr_t)out) & 7u) == 0, MNERF_E_ALIGN, "mnerf_lpips_sum: slots / out must be 8-byte aligned");
  lpips_sum_kernel<<<dim3(n_images), dim3(LP_THREADS), 0, (hipStream_t)stream>>>(slots, image_stride, n_slots, out);
  return mnerf_check_launch("mnerf_lpips_sum");
}

extern "C" int mnerf_lpips_vgg(const float* pred, const float* gt, int64_t gt_image_stride, const uint8_t* invalid_mask, int32_t n_images,
                               int32_t height, int32_t width, const mnerf_lpips_weights* weights, void* workspace, double* out,
                               void* stream) {
  const char* who = "mnerf_lpips_vgg";
  MNERF_REQUIRE(pred && gt && weights && workspace && out, MNERF_E_NULL, "%s: pred / gt / weights / workspace / out is NULL", who);
  for (int l = 0; l < LP_LAYERS; ++l)
    MNERF_REQUIRE(weights->wstream[l] && weights->bias[l], MNERF_E_NULL, "%s: weights of layer %d are NULL", who, l);
  for (int l = 0; l < LP_STAGES; ++l) MNERF_REQUIRE(weights->head[l], MNERF_E_NULL, "%s: head %d is NULL", who, l);
  MNERF_REQUIRE(n_images >= 1 && n_images <= 65535, MNERF_E_RANGE, "%s: n_images %d outside [1, 65535]", who, n_images);
  LpShape s;
  MNERF_REQUIRE(lp_shape(height, width, invalid_mask != nullptr, &s), MNERF_E_RANGE,
                "%s: %d x %d image, the processed image (%s) must be at least 16 x 16 (four 2x2 pools)", who, height, width,
                invalid_mask ? "the whole frame with a mask" : "the 80 % centre crop without a mask");
  MNERF_REQUIRE((int64_t)height * width <= INT32_MAX / 256, MNERF_E_RANGE, "%s: %d x %d image is too large", who, height, width);
  MNERF_REQUIRE(gt_image_stride >= (int64_t)3 * height * width, MNERF_E_RANGE,
                "%s: gt_image_stride %lld is less than one image (%lld floats)", who, (long long)gt_image_stride,
                (long long)3 * height * width);
  for (int l = 0; l < LP_LAYERS; ++l)
    MNERF_REQUIRE(mnerf_aligned16(weights->wstream[l]), MNERF_E_ALIGN, "%s: wstream of layer %d must be 16-byte aligned", who, l);
  MNERF_REQUIRE(mnerf_aligned16(workspace) && (((uintptr_t)out) & 7u) == 0, MNERF_E_ALIGN,
                "%s: workspace must be 16-byte aligned, out 8-byte aligned", who);

  const LpLayout L = lp_layout(s, n_images);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  float* act[2] = {(float*)base, (float*)(base + L.act_bytes)};
  char* images = base + 2 * L.act_bytes;
  const int64_t hw = (int64_t)s.ph * s.pw;
  // every absmax region of every pair starts at zero (producers merge with atomic maxima)
  for (int img = 0; img < n_images; ++img) {
    const hipError_t e = hipMemsetAsync(images + (int64_t)img * L.per_image + L.in_bytes, 0, (size_t)L.absmax_bytes, st);
    if (e != hipSuccess) {
      mnerf_set_error("%s: clearing the absmax regions failed: %s", who, hipGetErrorString(e));
      return (int)e;
    }
  }
  lpips_input_kernel<<<dim3((unsigned)((hw + LP_THREADS - 1) / LP_THREADS), n_images), dim3(LP_THREADS), 0, st>>>(
      pred, gt, gt_image_stride, invalid_mask, s, (float*)images, L.per_image / 4, L.in_bytes / 4);
  if (int rc = mnerf_check_launch("mnerf_lpips_vgg (input)")) return rc;

  const int64_t n_slots = lp_image_slots(s);
  for (int img = 0; img < n_images; ++img) {
    char* mine = images + (int64_t)img * L.per_image;
    float* regions = (float*)(mine + L.in_bytes);  // region 0: the input; region l + 1: the output of layer l
    double* slots = (double*)(mine + L.in_bytes + L.absmax_bytes);
    const float* cur = (const float*)mine;
    int h = s.ph, w = s.pw, stage = 0, flip = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
      mnerf_conv cv;
      cv.wstream = weights->wstream[l];
      cv.wstream_floats = mnerf_lpips_wstream_floats(l);
      cv.bias = weights->bias[l];
      cv.c_in = LP_CIN[l], cv.c_out = LP_COUT[l], cv.ksize = 3, cv.stride = 1;
      cv.ew = weights->ew[l];
      cv.leaky_slope = 0.0f;  // ReLU
      float* dst = act[flip];
      if (int rc = mnerf_conv2d(&cv, cur, 0, 0, regions + (int64_t)l * MNERF_ABSMAX_FLOATS, nullptr, nullptr, dst, MNERF_CONV_OUT_NCHW,
                                regions + (int64_t)(l + 1) * MNERF_ABSMAX_FLOATS, 2, h, w, st))
        return rc;
      cur = dst;
      flip ^= 1;
      if (l == LP_STAGE_END[stage]) {
        const int c = LP_STAGE_C[stage];
        if (int rc = lp_head(cur, cur + (int64_t)c * h * w, weights->head[stage], c, h, w, slots, st)) return rc;
        slots += lp_head_slots(h, w);
        if (++stage < LP_STAGES) {  // the pooled tensor keeps its producer's absmax region: a maximum cannot grow
          if (int rc = lp_maxpool(cur, act[flip], (int64_t)2 * c, h, w, st)) return rc;
          cur = act[flip];
          flip ^= 1;
          h >>= 1, w >>= 1;
        }
      }
    }
  }
  lpips_sum_kernel<<<dim3(n_images), dim3(LP_THREADS), 0, st>>>((const double*)(images + L.in_bytes + L.absmax_bytes), L.per_image / 8,
                                                                 (int)n_slots, out);
  return mnerf_check_launch(who);
}
