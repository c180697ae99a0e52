// The tail of a training iteration (gfx950): gradient norm per parameter group, gradient clipping + AdamW step over ALL
// parameter tensors in one launch, and the L2 loss with its gradient.
//
// Replaces (paths relative to the reference):
//   coach.py:36-38, 257   MSE_loss: (pred - label) ** 2 -> mean, and what autograd derives from it
//   coach.py:225-226      torch.nn.utils.clip_grad_norm_(feat_enc.parameters(), clip_enc)
//   coach.py:227          torch.optim.AdamW.step()
// torch runs the last two as a few hundred small foreach / element-wise launches (one list of 153 tensors from 1 to 262 144
// elements).  Here the tensors travel as a device table of rows (mnerf_optim_row); a workgroup finds its (tensor, chunk) by a
// binary search over the rows' first-block prefix, so one launch covers every tensor whatever its size.  All three kernels
// are streaming passes: 16-byte accesses where the four pointers of a row allow it, a scalar path for rows that are only
// 4-byte aligned and for the last numel % 4 elements.
//
// Data-parallel training adds two more streaming passes over the same table (ABI 11): grad_pack_kernel copies every gradient
// chunk into one contiguous bucket (chunk b of the table at float offset b * OPT_CHUNK, zeros behind numel, one last chunk of
// side slots), so that ONE collective sums the gradients of all ranks, and grad_unpack_kernel writes bucket * scale back.
//
// Reductions are deterministic: a workgroup reduces its chunk in a fixed shuffle / LDS order into one workspace slot, a
// second kernel adds the slots of a group in a fixed order (in double).  No floating-point atomics.
#include "common.hpp"

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = MNERF_OPTIM_CHUNK;  // elements of one (tensor, chunk) unit: 4 float4 per lane

struct OptGroupDev {
  double lr;
  float decay, beta2, one_minus_beta1, one_minus_beta2, eps, max_norm;
  int32_t block_begin, block_end;  // the group's workgroups (rows are sorted by group)
};
struct OptGroupsDev {
  int32_t n_groups;
  OptGroupDev g[MNERF_OPTIM_MAX_GROUPS];
};

// fixed-order sum over the workgroup; the result is valid in thread 0
__device__ __forceinline__ float opt_block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.0f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < OPT_THREADS / 64; ++i) t += red[i];
  }
  return t;
}

// row whose block range holds `block`: the last row with block_begin <= block
__device__ __forceinline__ int opt_find_row(const mnerf_optim_row* __restrict__ rows, int n_rows, int block) {
  int lo = 0, hi = n_rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].block_begin <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool opt_vec_ok(const mnerf_optim_row& r) {
  return (((uintptr_t)r.param | (uintptr_t)r.grad | (uintptr_t)r.exp_avg | (uintptr_t)r.exp_avg_sq) & 15u) == 0;
}

// ---- kernel 1: sum of squares of one chunk of one gradient -> partial[blockIdx.x]
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_partial_kernel(const mnerf_optim_row* __restrict__ rows, int n_rows,
                                                                         float* __restrict__ partial) {
  __shared__ float red[OPT_THREADS / 64];
  const int row = opt_find_row(rows, n_rows, (int)blockIdx.x);
  const mnerf_optim_row r = rows[row];
  const int64_t begin = (int64_t)((int)blockIdx.x - r.block_begin) * OPT_CHUNK;
  const int64_t left = r.numel - begin;
  const int n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
  const float* g = r.grad + begin;
  float s = 0.0f;
  if ((((uintptr_t)g) & 15u) == 0) {
    const int n4 = n >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
#pragma unroll
    for (int i = 0; i < OPT_CHUNK / 4 / OPT_THREADS; ++i) {
      const int j = i * OPT_THREADS + (int)threadIdx.x;
      if (j < n4) {
        const float4 v = g4[j];
        s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
      }
    }
    const int j = (n4 << 2) + (int)threadIdx.x;
    if (j < n) s += g[j] * g[j];
  } else {
    for (int j = (int)threadIdx.x; j < n; j += OPT_THREADS) s += g[j] * g[j];
  }
  const float t = opt_block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// ---- kernel 2: one workgroup per group adds that group's partials in a fixed order
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_final_kernel(OptGroupsDev groups, const float* __restrict__ partial,
                                                                       float* __restrict__ sumsq) {
  __shared__ double red[OPT_THREADS];
  const OptGroupDev g = groups.g[blockIdx.x];
  double s = 0.0;
  for (int j = g.block_begin + (int)threadIdx.x; j < g.block_end; j += OPT_THREADS) s += (double)partial[j];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int off = OPT_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sumsq[blockIdx.x] = (float)red[0];
}

// ---- kernel 3: clip + AdamW on one chunk of one tensor
struct AdamCoef {
  float clip, decay, one_minus_beta1, beta2, one_minus_beta2, eps, step_size, bc2_sqrt;
};

// The operations, their order and their roundings are those of torch's foreach AdamW (each foreach op rounds once; lerp, addcmul
// and addcdiv end in one fused multiply-add), so the two differ only through the clip coefficient's summation order.
__device__ __forceinline__ void adamw_element(float& p, float& g, float& m, float& v, const AdamCoef& c) {
  g *= c.clip;                                  // clip_grad_norm_: grad.mul_(clip_coef)
  p *= c.decay;                                 // param.mul_(1 - lr * weight_decay)
  m = fmaf(c.one_minus_beta1, g - m, m);        // exp_avg.lerp_(grad, 1 - beta1)
  v = fmaf(c.one_minus_beta2, g * g, v * c.beta2);  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  p = fmaf(-c.step_size, m / denom, p);         // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_step_kernel(const mnerf_optim_row* __restrict__ rows, int n_rows,
                                                                 OptGroupsDev groups, const float* __restrict__ sumsq) {
  const int row = opt_find_row(rows, n_rows, (int)blockIdx.x);
  const mnerf_optim_row r = rows[row];
  const int gi = min(max(r.group, 0), groups.n_groups - 1);
  const OptGroupDev gr = groups.g[gi];
  AdamCoef c;
  c.clip = 1.0f;
  if (gr.max_norm > 0.0f) {
    const float norm = sqrtf(sumsq[gi]);
    c.clip = fminf(gr.max_norm / (norm + 1e-6f), 1.0f);
  }
  const bool write_grad = c.clip != 1.0f;  // a coefficient of exactly 1 leaves the same bits
  c.decay = gr.decay;
  c.one_minus_beta1 = gr.one_minus_beta1;
  c.beta2 = gr.beta2;
  c.one_minus_beta2 = gr.one_minus_beta2;
  c.eps = gr.eps;
  c.step_size = (float)(gr.lr / r.bias_correction1);  // torch: lr / bias_correction1 in double, one rounding
  c.bc2_sqrt = r.bias_correction2_sqrt;
  const int64_t begin = (int64_t)((int)blockIdx.x - r.block_begin) * OPT_CHUNK;
  const int64_t left = r.numel - begin;
  const int n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
  float* p = r.param + begin;
  float* g = r.grad + begin;
  float* m = r.exp_avg + begin;
  float* v = r.exp_avg_sq + begin;
  int tail_from = 0;
  if (opt_vec_ok(r)) {  // begin is a multiple of OPT_CHUNK: the chunk is as aligned as the row
    const int n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
#pragma unroll
    for (int i = 0; i < OPT_CHUNK / 4 / OPT_THREADS; ++i) {
      const int j = i * OPT_THREADS + (int)threadIdx.x;
      if (j < n4) {
        float4 pp = p4[j], gg = g4[j], mm = m4[j], vv = v4[j];
        adamw_element(pp.x, gg.x, mm.x, vv.x, c);
        adamw_element(pp.y, gg.y, mm.y, vv.y, c);
        adamw_element(pp.z, gg.z, mm.z, vv.z, c);
        adamw_element(pp.w, gg.w, mm.w, vv.w, c);
        p4[j] = pp;
        m4[j] = mm;
        v4[j] = vv;
        if (write_grad) g4[j] = gg;
      }
    }
    tail_from = n4 << 2;
  }
  for (int j = tail_from + (int)threadIdx.x; j < n; j += OPT_THREADS) {
    float pp = p[j], gg = g[j], mm = m[j], vv = v[j];
    adamw_element(pp, gg, mm, vv, c);
    p[j] = pp;
    m[j] = mm;
    v[j] = vv;
    if (write_grad) g[j] = gg;
  }
}

// ---- data-parallel exchange: gradients -> bucket -> gradients.  Workgroup b < n_blocks owns bucket[b * OPT_CHUNK, +OPT_CHUNK):
// the bucket side of a chunk is 16-byte aligned whatever the gradient's own alignment, so the bucket is always accessed as float4.
// Workgroup n_blocks owns the chunk of side slots (the iteration's loss rides there: no collective of its own).
__global__ __launch_bounds__(OPT_THREADS) void grad_pack_kernel(const mnerf_optim_row* __restrict__ rows, int n_rows, int n_blocks,
                                                                const float* __restrict__ side, int n_side,
                                                                float* __restrict__ bucket) {
  float4* out4 = reinterpret_cast<float4*>(bucket + (int64_t)blockIdx.x * OPT_CHUNK);
  const float* g;
  int n;
  if ((int)blockIdx.x < n_blocks) {
    const int row = opt_find_row(rows, n_rows, (int)blockIdx.x);
    const mnerf_optim_row r = rows[row];
    const int64_t begin = (int64_t)((int)blockIdx.x - r.block_begin) * OPT_CHUNK;
    const int64_t left = r.numel - begin;
    n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
    g = r.grad + begin;
  } else {  // the side chunk
    g = side;
    n = side ? n_side : 0;
  }
  const bool vec = (((uintptr_t)g) & 15u) == 0;
#pragma unroll
  for (int i = 0; i < OPT_CHUNK / 4 / OPT_THREADS; ++i) {
    const int j = i * OPT_THREADS + (int)threadIdx.x;
    const int e = j << 2;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // behind numel the bucket holds zeros: nothing uninitialised is summed
    if (vec && e + 3 < n) {
      v = reinterpret_cast<const float4*>(g)[j];
    } else {  // a gradient that is only 4-byte aligned, and the last numel % 4 elements
      if (e < n) v.x = g[e];
      if (e + 1 < n) v.y = g[e + 1];
      if (e + 2 < n) v.z = g[e + 2];
      if (e + 3 < n) v.w = g[e + 3];
    }
    out4[j] = v;
  }
}

__global__ __launch_bounds__(OPT_THREADS) void grad_unpack_kernel(const mnerf_optim_row* __restrict__ rows, int n_rows, int n_blocks,
                                                                  const float* __restrict__ bucket, float scale,
                                                                  float* __restrict__ side_out, int n_side) {
  const float4* in4 = reinterpret_cast<const float4*>(bucket + (int64_t)blockIdx.x * OPT_CHUNK);
  float* g;
  int n;
  if ((int)blockIdx.x < n_blocks) {
    const int row = opt_find_row(rows, n_rows, (int)blockIdx.x);
    const mnerf_optim_row r = rows[row];
    const int64_t begin = (int64_t)((int)blockIdx.x - r.block_begin) * OPT_CHUNK;
    const int64_t left = r.numel - begin;
    n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
    g = r.grad + begin;
  } else {
    g = side_out;
    n = n_side;
  }
  const bool vec = (((uintptr_t)g) & 15u) == 0;
#pragma unroll
  for (int i = 0; i < OPT_CHUNK / 4 / OPT_THREADS; ++i) {
    const int j = i * OPT_THREADS + (int)threadIdx.x;
    const int e = j << 2;
    if (e >= n) continue;
    float4 v = in4[j];
    v.x *= scale, v.y *= scale, v.z *= scale, v.w *= scale;  // one fp32 multiply per element: torch's flat.mul_(scale)
    if (vec && e + 3 < n) {
      reinterpret_cast<float4*>(g)[j] = v;
    } else {
      g[e] = v.x;
      if (e + 1 < n) g[e + 1] = v.y;
      if (e + 2 < n) g[e + 2] = v.z;
      if (e + 3 < n) g[e + 3] = v.w;
    }
  }
}

// ---- L2 loss: ONE workgroup (the loss of a training iteration has rand_rays_train x 3 terms), fixed-order sum
constexpr int L2_THREADS = 1024;

__global__ __launch_bounds__(L2_THREADS) void l2_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             int64_t n, float weight, float* __restrict__ loss,
                                                             float* __restrict__ grad) {
  __shared__ float red[L2_THREADS / 64];
  const float inv_n = 1.0f / (float)n;
  const float gs = 2.0f * weight * inv_n;
  float s = 0.0f;
  const bool vec = ((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)grad) & 15u) == 0);
  int64_t tail_from = 0;
  if (vec) {
    const int64_t n4 = n >> 2;
    const float4* a4 = reinterpret_cast<const float4*>(pred);
    const float4* b4 = reinterpret_cast<const float4*>(target);
    float4* g4 = reinterpret_cast<float4*>(grad);
    for (int64_t j = threadIdx.x; j < n4; j += L2_THREADS) {
      const float4 a = a4[j], b = b4[j];
      const float4 d = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
      s += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
      if (grad) g4[j] = make_float4(gs * d.x, gs * d.y, gs * d.z, gs * d.w);
    }
    tail_from = n4 << 2;
  }
  for (int64_t j = tail_from + threadIdx.x; j < n; j += L2_THREADS) {
    const float d = pred[j] - target[j];
    s += d * d;
    if (grad) grad[j] = gs * d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < L2_THREADS / 64; ++i) t += red[i];
    loss[0] = weight * (t * inv_n);
  }
}

int opt_groups(const char* what, const mnerf_optim_group* groups, int32_t n_groups, int32_t n_blocks, OptGroupsDev* out) {
  MNERF_REQUIRE(groups != nullptr, MNERF_E_NULL, "%s: groups is NULL", what);
  MNERF_REQUIRE(n_groups >= 1 && n_groups <= MNERF_OPTIM_MAX_GROUPS, MNERF_E_RANGE, "%s: n_groups %d outside [1, %d]", what,
                n_groups, MNERF_OPTIM_MAX_GROUPS);
  out->n_groups = n_groups;
  int32_t at = 0;
  for (int i = 0; i < n_groups; ++i) {
    const mnerf_optim_group& g = groups[i];
    MNERF_REQUIRE(g.n_blocks >= 0, MNERF_E_RANGE, "%s: group %d has n_blocks %d", what, i, g.n_blocks);
    OptGroupDev& d = out->g[i];
    d.lr = g.lr;
    d.decay = (float)(1.0 - g.lr * g.weight_decay);
    d.beta2 = (float)g.beta2;
    d.one_minus_beta1 = (float)(1.0 - g.beta1);
    d.one_minus_beta2 = (float)(1.0 - g.beta2);
    d.eps = (float)g.eps;
    d.max_norm = (float)g.max_norm;
    d.block_begin = at;
    at += g.n_blocks;
    d.block_end = at;
  }
  MNERF_REQUIRE(at == n_blocks, MNERF_E_RANGE, "%s: the groups' n_blocks add up to %d, n_blocks is %d", what, at, n_blocks);
  return MNERF_OK;
}

int opt_table(const char* what, const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks) {
  MNERF_REQUIRE(rows != nullptr, MNERF_E_NULL, "%s: rows is NULL", what);
  MNERF_REQUIRE(n_rows >= 1 && n_blocks >= n_rows, MNERF_E_RANGE, "%s: n_rows %d, n_blocks %d (every row has a block)", what,
                n_rows, n_blocks);
  MNERF_REQUIRE((((uintptr_t)rows) & 15u) == 0, MNERF_E_ALIGN, "%s: rows must be 16-byte aligned", what);
  return MNERF_OK;
}

int opt_bucket(const char* what, const float* bucket, int32_t n_side) {
  MNERF_REQUIRE(bucket != nullptr, MNERF_E_NULL, "%s: bucket is NULL", what);
  MNERF_REQUIRE((((uintptr_t)bucket) & 15u) == 0, MNERF_E_ALIGN, "%s: bucket must be 16-byte aligned", what);
  MNERF_REQUIRE(n_side >= 0 && n_side <= OPT_CHUNK, MNERF_E_RANGE, "%s: n_side %d outside [0, %d]", what, n_side, OPT_CHUNK);
  return MNERF_OK;
}

}  // namespace

extern "C" int64_t mnerf_optim_row_blocks(int64_t numel) { return numel <= 0 ? -1 : (numel + OPT_CHUNK - 1) / OPT_CHUNK; }

extern "C" int mnerf_grad_sumsq(const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks, const mnerf_optim_group* groups,
                                int32_t n_groups, float* workspace, float* sumsq, void* stream) {
  if (int rc = opt_table("mnerf_grad_sumsq", rows, n_rows, n_blocks)) return rc;
  OptGroupsDev gd;
  if (int rc = opt_groups("mnerf_grad_sumsq", groups, n_groups, n_blocks, &gd)) return rc;
  MNERF_REQUIRE(workspace && sumsq, MNERF_E_NULL, "mnerf_grad_sumsq: workspace / sumsq is NULL");
  hipStream_t st = (hipStream_t)stream;
  grad_sumsq_partial_kernel<<<dim3(n_blocks), dim3(OPT_THREADS), 0, st>>>(rows, n_rows, workspace);
  if (int rc = mnerf_check_launch("mnerf_grad_sumsq (partial sums)")) return rc;
  grad_sumsq_final_kernel<<<dim3(n_groups), dim3(OPT_THREADS), 0, st>>>(gd, workspace, sumsq);
  return mnerf_check_launch("mnerf_grad_sumsq");
}

extern "C" int mnerf_adamw_step(const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks, const mnerf_optim_group* groups,
                                int32_t n_groups, const float* sumsq, void* stream) {
  if (int rc = opt_table("mnerf_adamw_step", rows, n_rows, n_blocks)) return rc;
  OptGroupsDev gd;
  if (int rc = opt_groups("mnerf_adamw_step", groups, n_groups, n_blocks, &gd)) return rc;
  bool clips = false;
  for (int i = 0; i < n_groups; ++i) clips = clips || gd.g[i].max_norm > 0.0f;
  MNERF_REQUIRE(!clips || sumsq, MNERF_E_NULL, "mnerf_adamw_step: a group clips (max_norm > 0) but sumsq is NULL");
  adamw_step_kernel<<<dim3(n_blocks), dim3(OPT_THREADS), 0, (hipStream_t)stream>>>(rows, n_rows, gd, sumsq);
  return mnerf_check_launch("mnerf_adamw_step");
}

extern "C" int mnerf_l2_loss(const float* pred, const float* target, int64_t n, float weight, float* loss, float* grad,
                             void* stream) {
  MNERF_REQUIRE(pred && target && loss, MNERF_E_NULL, "mnerf_l2_loss: pred / target / loss is NULL");
  MNERF_REQUIRE(n >= 1, MNERF_E_RANGE, "mnerf_l2_loss: n = %lld", (long long)n);
  l2_loss_kernel<<<dim3(1), dim3(L2_THREADS), 0, (hipStream_t)stream>>>(pred, target, n, weight, loss, grad);
  return mnerf_check_launch("mnerf_l2_loss");
}

extern "C" int64_t mnerf_grad_bucket_floats(int64_t n_blocks) {
  return n_blocks < 1 || n_blocks >= INT32_MAX ? -1 : (n_blocks + 1) * OPT_CHUNK;
}

extern "C" int mnerf_grad_pack(const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks, const float* side, int32_t n_side,
                               float* bucket, void* stream) {
  if (int rc = opt_table("mnerf_grad_pack", rows, n_rows, n_blocks)) return rc;
  if (int rc = opt_bucket("mnerf_grad_pack", bucket, n_side)) return rc;
  MNERF_REQUIRE(side != nullptr || n_side == 0, MNERF_E_NULL, "mnerf_grad_pack: side is NULL with n_side %d", n_side);
  grad_pack_kernel<<<dim3(n_blocks + 1), dim3(OPT_THREADS), 0, (hipStream_t)stream>>>(rows, n_rows, n_blocks, side, n_side, bucket);
  return mnerf_check_launch("mnerf_grad_pack");
}

extern "C" int mnerf_grad_unpack(const mnerf_optim_row* rows, int32_t n_rows, int32_t n_blocks, const float* bucket, float scale,
                                 float* side_out, int32_t n_side, void* stream) {
  if (int rc = opt_table("mnerf_grad_unpack", rows, n_rows, n_blocks)) return rc;
  if (int rc = opt_bucket("mnerf_grad_unpack", bucket, n_side)) return rc;
  MNERF_REQUIRE(side_out != nullptr || n_side == 0, MNERF_E_NULL, "mnerf_grad_unpack: side_out is NULL with n_side %d", n_side);
  const int grid = n_blocks + (n_side > 0 ? 1 : 0);
  grad_unpack_kernel<<<dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream>>>(rows, n_rows, n_blocks, bucket, scale, side_out, n_side);
  return mnerf_check_launch("mnerf_grad_unpack");
}
