// K3+K4+K5 — conditional radiance MLP + per-ray transformer + alpha compositing as ONE ray-chunk kernel for gfx950: what the
// decoder's two kernels and two objects share.
//
// Replaces, per chunk of rays (paths in the reference implementation):
//   models/matchnerf.py:118-132        NDC warp w.r.t. source view 0, view-dir rotation
//   models/rfdecoder/cond_nerf.py:52-100   CondNeRF.forward (posenc, FiLM-modulated MLP, heads)
//   models/rfdecoder/ray_transformer.py:14-26, 49-79   4-head attention along the ray + LN
//   models/rfdecoder/nerf.py:101-124   NeRF.composite
// The reference runs these as ~60 eager ops that materialise [R,S,128] activations per layer (134 MB each at R=4096,S=64) and a
// [R,4,S,S] score tensor (268 MB).  Here a workgroup owns a tile of whole rays, activations never leave registers, the
// ray-attention K/V and per-sample (rgb,sigma) live in LDS, and only 5 floats per ray are written to HBM.
//
// Two kernels evaluate it, one per file:
//   decoder.hip          decoder_pp_kernel<SP,FS,POSES,NPK>: the ping-pong form of the split-fp16 ("f16x3") matrix path, the default
//                        since round 3 for the shipped decoder shape; and the library's decoder entry points
//   decoder_staged.hpp   decoder_kernel<NW,SP,FMT,CVF>: the staged form - every other shape and weight-stream format (FMT 0 exact f32,
//                        1 bf16x6, 2 f16x3), and with CVF = 1 the one-launch form with the cost-volume walk inside
//                        (decoder_fused.hip, a separate object)
// This header: the weight-segment constants and DecSched, the timeline stamps of the MNERF_TIMELINE build, the device helpers of the
// three matrix paths and, on the host side, the weight schedule (shared with the Python packers) and the entry points' argument checks.
#pragma once
#include <stdlib.h>

#include "cv_walk.hpp"
#include "split_f16.hpp"

#define SEG_CAP_FLOATS (33 * 256)  // one LDS weight buffer: 33 KiB
#define MAX_SEGS 64
#define SMALL_FIXED 32    // floats of `small` (LayerNorm weight | bias) before the ray-posenc table
// tail segment (resident across the attention phase): float offsets of its sub-stages
#define TAIL_QKV 0
#define TAIL_FCO 1024
#define TAIL_OA0 1536
#define TAIL_OA2 2112
#define TAIL_FLOATS 2688

#ifdef MNERF_TIMELINE
// debug build (tools/exp/timeline.py): per-wave s_memtime stamps at phase boundaries
#define TL_POINTS 20
#define TL_STAMP(k)                                                                     \
  do {                                                                                  \
    if (sch.tl && lane == 0 && tl_slot >= 0 && tl_tile < 4)                             \
      sch.tl[(((size_t)tl_slot * 4 + tl_tile) * NW + wave) * TL_POINTS + (k)] =         \
          __builtin_amdgcn_s_memtime();                                                 \
  } while (0)
#else
#define TL_STAMP(k) do {} while (0)
#endif

struct DecSched {
#ifdef MNERF_TIMELINE
  unsigned long long* tl;
#endif
#ifdef MNERF_FUSED_DEBUG
  // debug build of the one-launch form (tools/exp/race_probe.py): what the trunk consumed, where each tile ran
  unsigned dbg_flags;   // 2 drain DMA + barrier before the walk, 4 first weight segment requested after the walk,
                        // 8 full wait + barrier after the FiLM inputs are read, 32 NaN-poison of the walk's LDS,
                        // 64 weight segments copied with plain loads + LDS stores instead of LDS-DMA
  float* dbg_rows;      // [rays*S][32] conditioning inputs as read by the trunk
  float* dbg_nv;        // [rays*S] mask sum as read by the trunk
  unsigned* dbg_tile;   // [tiles][4] blockIdx, HW_ID, XCC_ID, low clock word
#endif
  int stagger_sleeps;  // one-time start delay (x s_sleep 127) of the 2nd resident workgroup of a CU
  int stagger_mode;    // which workgroups wait: 0 odd HW wave slot, 1 upper half of grid, 2 (b>>3)&1, 3 all
  int n_seg;
  int film_steps, enc_steps;
  int seg_off[MAX_SEGS];     // float offset of the segment in wstream (multiple of 256)
  int seg_floats[MAX_SEGS];  // padded to a multiple of 256 floats (1 KiB DMA pieces)
  int seg_steps[MAX_SEGS];
};

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

template <int NW>
__device__ __forceinline__ void prefetch_segment(const float* __restrict__ wstream,
                                                 const DecSched& sch, int seg, unsigned base /* LDS byte address */,
                                                 int wave, int lane) {
  if (seg >= sch.n_seg) return;
  const float* src = wstream + sch.seg_off[seg] + lane * 4;
  const int pieces = sch.seg_floats[seg] >> 8;
#ifdef MNERF_FUSED_DEBUG
  if (sch.dbg_flags & 64u) {  // no LDS-DMA at all: plain loads + LDS stores (compiler-tracked)
    typedef v4f32 __attribute__((address_space(3)))* lds_v4f32_ptr;
    for (int p = wave; p < pieces; p += NW) {
      const v4f32 t = *reinterpret_cast<const v4f32*>(src + p * 256);
      *((lds_v4f32_ptr)(size_t)(base + (unsigned)p * 1024u + (unsigned)lane * 16u)) = t;
    }
    return;
  }
#endif
  for (int p = wave; p < pieces; p += NW)
    glds16(src + p * 256, __builtin_amdgcn_readfirstlane(base + (unsigned)p * 1024u));
}

// one K-step against 4 / 2 / 1 M-blocks; A fragments laid out [step][lane][nmb]
__device__ __forceinline__ void step4(f32x16 (&acc)[4], const float* seg, int step, int lane,
                                      float b) {
  const float4 a = reinterpret_cast<const float4*>(seg)[step * 64 + lane];
  acc[0] = mfma(a.x, b, acc[0]);
  acc[1] = mfma(a.y, b, acc[1]);
  acc[2] = mfma(a.z, b, acc[2]);
  acc[3] = mfma(a.w, b, acc[3]);
}
__device__ __forceinline__ void step2(f32x16 (&acc)[2], const float* seg, int step, int lane,
                                      float b) {
  const float2 a = reinterpret_cast<const float2*>(seg)[step * 64 + lane];
  acc[0] = mfma(a.x, b, acc[0]);
  acc[1] = mfma(a.y, b, acc[1]);
}
__device__ __forceinline__ void step1(f32x16& acc, const float* seg, int step, int lane, float b) {
  acc = mfma(seg[step * 64 + lane], b, acc);
}

// 32 K-steps fed from two 16-register accumulator blocks of the previous layer
template <int NMB>
__device__ __forceinline__ void steps_from_regs(f32x16 (&acc)[NMB], const float* seg, int step0,
                                                int lane, const f32x16& h0, const f32x16& h1);
template <>
__device__ __forceinline__ void steps_from_regs<4>(f32x16 (&acc)[4], const float* seg, int step0,
                                                   int lane, const f32x16& h0, const f32x16& h1) {
  // A fragments are double-buffered in registers: the ds_read_b128 of step t+1 is issued before
  // the four MFMAs of step t, so its LDS latency hides under 256 cycles of matrix work.
  const float4* a4 = reinterpret_cast<const float4*>(seg) + step0 * 64 + lane;
  float4 cur = a4[0];
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    const float4 nxt = a4[(r + 1) * 64];  // r == 31 reads the following fragment (bias step or pad)
    __builtin_amdgcn_sched_barrier(0);    // keep the prefetch ABOVE this step's MFMAs
    const float b = r < 16 ? h0[r & 15] : h1[r & 15];
    acc[0] = mfma(cur.x, b, acc[0]);
    acc[1] = mfma(cur.y, b, acc[1]);
    acc[2] = mfma(cur.z, b, acc[2]);
    acc[3] = mfma(cur.w, b, acc[3]);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
  }
}
// 16 pipelined K-steps against 4 M-blocks fed from one 16-register block
__device__ __forceinline__ void steps16_from_regs(f32x16 (&acc)[4], const float* seg, int step0, int lane,
                                                  const f32x16& e) {
  const float4* a4 = reinterpret_cast<const float4*>(seg) + step0 * 64 + lane;
  float4 cur = a4[0];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float4 nxt = a4[(r + 1) * 64];
    __builtin_amdgcn_sched_barrier(0);
    acc[0] = mfma(cur.x, e[r], acc[0]);
    acc[1] = mfma(cur.y, e[r], acc[1]);
    acc[2] = mfma(cur.z, e[r], acc[2]);
    acc[3] = mfma(cur.w, e[r], acc[3]);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
  }
}

template <>
__device__ __forceinline__ void steps_from_regs<2>(f32x16 (&acc)[2], const float* seg, int step0,
                                                   int lane, const f32x16& h0, const f32x16& h1) {
#pragma unroll
  for (int r = 0; r < 16; ++r) step2(acc, seg, step0 + r, lane, h0[r]);
#pragma unroll
  for (int r = 0; r < 16; ++r) step2(acc, seg, step0 + 16 + r, lane, h1[r]);
}
template <>
__device__ __forceinline__ void steps_from_regs<1>(f32x16 (&acc)[1], const float* seg, int step0,
                                                   int lane, const f32x16& h0, const f32x16& h1) {
#pragma unroll
  for (int r = 0; r < 16; ++r) step1(acc[0], seg, step0 + r, lane, h0[r]);
#pragma unroll
  for (int r = 0; r < 16; ++r) step1(acc[0], seg, step0 + 16 + r, lane, h1[r]);
}

// B operand of positional-encoding step t for this lane (cond_nerf.py:108-116 legacy /
// nerf.py:126-133 non-legacy; the packer maps weight columns accordingly):
//   t < 3L : arg = x_{t%3} * 2^{t/3} (* pi)  ->  lower half sin(arg), upper half cos(arg)
//   t = 3L : (x | y)      t = 3L+1 : (z | 1)   [the 1 multiplies the packed bias column]
__device__ __forceinline__ float enc_operand(int t, int L3, int hl, float x, float y, float z,
                                             float freq_mul) {
  if (t < L3) {
    const int l = t / 3, c = t - 3 * l;
    const float xc = (c == 0) ? x : ((c == 1) ? y : z);
    const float arg = xc * (ldexpf(1.0f, l) * freq_mul);
    return sin_quarter(arg, hl);
  }
  if (t == L3) return hl ? y : x;
  return hl ? 1.0f : z;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
// 16 independent 4x4 outer products per wave: D[r](lane l) += A(lane 4*(l/4)+r) * B(lane l)
// (layout verified on MI355X, tools/exp/mfma4x4.hip)
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}

// 16 consecutive positional-encoding operands (steps t0 .. t0+15) evaluated into registers, so
// that the MFMA loop that consumes them is the same software-pipelined loop as a hidden layer.
// L_3D = 10 (every shipped config) is a compile-time case: with a run-time L every one of the 64 operand slots of a
// tile carries three comparisons against L whose results the compiler hoists out of the tile loop as exec-sized
// masks - ~300 spilled SGPRs, one v_readlane + v_cndmask per use (12 % of the kernel's VALU issue slots).
struct EncBase {   // x_c * freq_mul / (2 pi) as two floats per coordinate (exactly scalable by 2^l)
  float th[3], tl[3];
};
__device__ __forceinline__ EncBase enc_base(float x, float y, float z, float freq_mul) {
  EncBase b;
  turns_two_float(x * freq_mul, b.th[0], b.tl[0]);
  turns_two_float(y * freq_mul, b.th[1], b.tl[1]);
  turns_two_float(z * freq_mul, b.th[2], b.tl[2]);
  return b;
}
template <int T0>
__device__ __forceinline__ f32x16 enc_block16_L10(const EncBase& b, int hl, float x, float y, float z) {
  constexpr int L3 = 30;
  f32x16 e;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int t = T0 + i;
    if (t < L3) {
      const int l = t / 3, c = t - 3 * l;
      const float sc = (float)(1 << l);
      e[i] = sin_quarter_turns(b.th[c] * sc, b.tl[c] * sc, hl);
    } else if (t == L3) {
      e[i] = hl ? y : x;
    } else {
      e[i] = hl ? 1.0f : z;
    }
  }
  return e;
}

// ---------------------------------------------------------------- split-bf16 matrix path ("bf16x6")
// bf16x8, pk_bf16, Parts, split8 and mfma16 (the three-term split and its matrix instruction) live in split_f16.hpp.

// accumulators <- fp32 bias fragment [half][4][16] (exact fp32 biases, no K-step spent on them)
// LDS operands of the split-bf16 path are addressed by LDS byte offset through explicit address_space(3)
// pointers made from integers.

template <int NMB>
__device__ __forceinline__ void bias_init(f32x16 (&acc)[NMB], unsigned frag_lds, int hl) {
  lds_v4f32_cptr p = (lds_v4f32_cptr)(size_t)frag_lds + hl * 16;
#pragma unroll
  for (int m = 0; m < NMB; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const v4f32 t = p[m * 4 + q];
      acc[m][4 * q] = t.x;
      acc[m][4 * q + 1] = t.y;
      acc[m][4 * q + 2] = t.z;
      acc[m][4 * q + 3] = t.w;
    }
}

// NS K16-steps against NMB output blocks.  `base`: fragments [step][block][hi|mid|lo][64 lanes][8 bf16];
// v: the lane's 8*NS operands.  A fragments of unit (step, block) i+1 are read before the six MFMAs
// of unit i (192 cycles of matrix work hide the LDS latency).
template <int NMB, int NS>
__device__ __forceinline__ void ksteps(f32x16 (&acc)[NMB], unsigned base_lds, int lane, const float (&v)[8 * NS]) {
  lds_u32x4_cptr a = (lds_u32x4_cptr)(size_t)base_lds + lane;
  u32x4 ch = a[0], cm = a[64], cl = a[128];
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    float vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) vv[j] = v[8 * u + j];
    const Parts b = split8(vv);
#pragma unroll
    for (int m = 0; m < NMB; ++m) {
      const int i = u * NMB + m;
      const int nx = (i + 1 < NS * NMB) ? (i + 1) * 192 : i * 192;  // the last unit re-reads itself
      const u32x4 nh = a[nx], nm = a[nx + 64], nl = a[nx + 128];
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8 ah = __builtin_bit_cast(bf16x8, ch), am = __builtin_bit_cast(bf16x8, cm),
                   al = __builtin_bit_cast(bf16x8, cl);
      acc[m] = mfma16(ah, b.lo, acc[m]);
      acc[m] = mfma16(al, b.hi, acc[m]);
      acc[m] = mfma16(am, b.mid, acc[m]);
      acc[m] = mfma16(ah, b.mid, acc[m]);
      acc[m] = mfma16(am, b.hi, acc[m]);
      acc[m] = mfma16(ah, b.hi, acc[m]);
      __builtin_amdgcn_sched_barrier(0);
      ch = nh;
      cm = nm;
      cl = nl;
    }
  }
}

// two K16-steps fed from one 16-register block (an accumulator block of the previous layer)
template <int NMB>
__device__ __forceinline__ void kblock(f32x16 (&acc)[NMB], unsigned base_lds, int lane, const f32x16& h) {
  float v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = h[r];
  ksteps<NMB, 2>(acc, base_lds, lane, v);
}
#define K16_UNIT_BYTES 3072  // one (step, block): hi | mid | lo fragments

// Experiment knob, OFF: streaming the conditioning rows with non-temporal stores (cost volume) and loads (here).
// Measured on MI355X (profiles/r2_nt_*): HBM-side counters unchanged (the scratch lines it was meant to protect are
// written back either way), cost volume 9.8 -> 11.2 ms, decoder unchanged.  The write-then-read pair of the staged
// form is served best by the default cache policy.
__device__ __forceinline__ float4 ld_stream4(const float* p, bool lds) {
  return *reinterpret_cast<const float4*>(p);
}

// ------------------------------------------------------------------ host side
// Segment schedules shared with the Python packers (matchnerf_amd/cond_nerf.py).
static void finish_schedule(DecSched* sch, int n, int film_steps, int enc_steps) {
  sch->n_seg = n;
#ifdef MNERF_TIMELINE
  sch->tl = nullptr;
  if (const char* e = getenv("MNERF_TIMELINE_PTR")) sch->tl = (unsigned long long*)strtoull(e, nullptr, 0);
#endif
#ifdef MNERF_FUSED_DEBUG
  {
    auto envp = [](const char* k) -> unsigned long long {
      const char* e = getenv(k);
      return (e && *e) ? strtoull(e, nullptr, 0) : 0ull;
    };
    sch->dbg_flags = (unsigned)envp("MNERF_FDBG_FLAGS");
    sch->dbg_rows = (float*)envp("MNERF_FDBG_ROWS");
    sch->dbg_nv = (float*)envp("MNERF_FDBG_NV");
    sch->dbg_tile = (unsigned*)envp("MNERF_FDBG_TILE");
  }
#endif
  sch->stagger_sleeps = mnerf_tune().decoder_stagger;  // ~130k cycles ~ half a tile
  sch->stagger_mode = mnerf_tune().decoder_stagger_mode;
  sch->film_steps = film_steps;
  sch->enc_steps = enc_steps;
}

// split formats (bf16x3: PARTS = 3, fp16x2: PARTS = 2): stages (blocks, K16-steps per segment, header)
static int build_schedule_split(const mnerf_decoder* D, DecSched* sch, int parts) {
  const int tf = (D->cond_dim + 15) / 16, te = (3 * D->L_3D + 2 + 7) / 8;
  const int per = parts == 3 ? 2 : 4;  // K16-steps per segment of a 4-block stage (<= 33 KiB with the header)
  int n = 0;
  long long off = 0;
  auto add = [&](int nmb, int steps, bool hdr) -> bool {
    if (n >= MAX_SEGS - 1) return false;
    const int fl = (steps * nmb * parts + (hdr ? 1 : 0)) * 256;
    if (fl > SEG_CAP_FLOATS) return false;
    sch->seg_off[n] = (int)off;
    sch->seg_floats[n] = fl;
    sch->seg_steps[n] = steps;
    off += fl;
    ++n;
    return true;
  };
  auto add_chunks = [&](int t, bool hdr) -> bool {  // stage of 4 blocks cut into segments of `per` K16-steps
    for (int k = 0; k < t; k += per)
      if (!add(4, (t - k) >= per ? per : (t - k), hdr && k == 0)) return false;
    return true;
  };
  bool ok = add_chunks(tf, true) && add_chunks(te, true);
  for (int l = 1; l <= 4 && ok; ++l) ok = add_chunks(8, true);
  ok = ok && add_chunks(te, true) && add_chunks(8, false);  // l5e, l5h
  ok = ok && add(1, 8, true);                               // alpha
  ok = ok && add_chunks(8, true);                           // feature
  ok = ok && add(2, 4, true) && add(2, 5, false);           // views
  ok = ok && add(1, 4, true);                               // rgb
  if (!ok) return -1;
  const int fl = ((TAIL_FLOATS + 255) / 256) * 256;  // f32 tail: [w_qs;w_ks;w_vs | fc | out_alpha.0 | out_alpha.2]
  sch->seg_off[n] = (int)off;
  sch->seg_floats[n] = fl;
  sch->seg_steps[n] = 0;
  off += fl;
  ++n;
  finish_schedule(sch, n, tf, te);
  return (int)off;
}

// f32 format: a stage is cut into ceil(T/cap) segments, the first ones get floor(T/nseg) steps, the last one the
// rest; every segment is padded to a multiple of 256 floats.
static int build_schedule(const mnerf_decoder* D, DecSched* sch) {
  if (D->wstream_format == MNERF_WSTREAM_BF16X3) return build_schedule_split(D, sch, 3);
  if (D->wstream_format == MNERF_WSTREAM_F16X2 || D->wstream_format == MNERF_WSTREAM_F16X1) return build_schedule_split(D, sch, 2);
  const int fs = D->cond_stride / 2, es = 3 * D->L_3D + 2;
  // film, l0, l1..l4, l5-enc, l5-h, feature, views, rgb, alpha (+ the resident tail segment)
  const int T[12] = {fs, es, 65, 65, 65, 65, es, 64, 65, 66, 33, 65};
  const int M[12] = {4, 4, 4, 4, 4, 4, 4, 4, 4, 2, 1, 1};
  int n = 0;
  long long off = 0;
  for (int st = 0; st < 12; ++st) {
    const int cap = SEG_CAP_FLOATS / (64 * M[st]);
    const int nseg = (T[st] + cap - 1) / cap;
    const int base = T[st] / nseg;
    for (int k = 0; k < nseg; ++k) {
      if (n >= MAX_SEGS) return -1;
      const int steps = (k == nseg - 1) ? (T[st] - base * (nseg - 1)) : base;
      const int fl = ((steps * 64 * M[st] + 255) / 256) * 256;
      if (fl > SEG_CAP_FLOATS) return -1;
      sch->seg_off[n] = (int)off;
      sch->seg_floats[n] = fl;
      sch->seg_steps[n] = steps;
      off += fl;
      ++n;
    }
  }
  {  // tail: [w_qs;w_ks;w_vs | fc | out_alpha.0 | out_alpha.2]
    if (n >= MAX_SEGS) return -1;
    const int fl = ((TAIL_FLOATS + 255) / 256) * 256;
    sch->seg_off[n] = (int)off;
    sch->seg_floats[n] = fl;
    sch->seg_steps[n] = 0;
    off += fl;
    ++n;
  }
  finish_schedule(sch, n, fs, es);
  return (int)off;
}

static bool known_format(int f) {
  return f == MNERF_WSTREAM_F32 || f == MNERF_WSTREAM_BF16X3 || f == MNERF_WSTREAM_F16X2 || f == MNERF_WSTREAM_F16X1;
}

static int pick_padded_samples(int S) {
  if (S <= 32) return 32;
  if (S <= 64) return 64;
  if (S <= 128) return 128;
  if (S <= 256) return 256;
  return -1;
}

// The arguments of one decoder launch as the entry points hand them on: mnerf_decoder_chunk (rays rebuilt in-kernel, composited
// outputs), mnerf_decoder_samples (caller-supplied sample coordinates / directions, per-sample outputs only) and the one-launch
// form of mnerf_render_chunk (fused_scene set, no cond).
struct DecCall {
  const char* who;
  const mnerf_decoder* dec;
  const mnerf_view* view0;
  const mnerf_rays* rays;
  const float* cond;
  float *rgb, *depth, *opacity, *rgb_s, *sigma;
  const float *ext_ndc, *ext_dir;
  const mnerf_scene* fused_scene;
  void* stream;
};

// The argument checks every form shares -> MNERF_OK with the padded sample count and the weight schedule, or the error.
static int check_decoder_call(const DecCall& c, int* Sp_out, DecSched* sch) {
  const char* who = c.who;
  const mnerf_decoder* dec = c.dec;
  const mnerf_rays* rays = c.rays;
  MNERF_REQUIRE(dec->wstream && dec->small_ && (c.cond || c.fused_scene), MNERF_E_NULL, "%s: NULL buffer", who);
  MNERF_REQUIRE(mnerf_aligned16(dec->wstream) && mnerf_aligned16(c.cond), MNERF_E_ALIGN,
                "%s: wstream / cond must be 16-byte aligned", who);
  MNERF_REQUIRE(dec->L_3D >= 0 && dec->L_3D <= 16, MNERF_E_RANGE, "%s: L_3D=%d", who, dec->L_3D);
  MNERF_REQUIRE(known_format(dec->wstream_format), MNERF_E_UNSUPPORTED, "%s: wstream_format=%d", who,
                dec->wstream_format);
  const int cs_max = dec->wstream_format == MNERF_WSTREAM_F32 ? MNERF_COND_STRIDE_MAX_F32 : MNERF_COND_STRIDE_MAX;
  MNERF_REQUIRE(dec->cond_stride % 8 == 0 && dec->cond_stride >= dec->cond_dim + 1 && dec->cond_stride <= cs_max,
                MNERF_E_RANGE, "%s: cond_stride=%d (cond_dim=%d) must be a multiple of 8 in (cond_dim, %d]", who,
                dec->cond_stride, dec->cond_dim, cs_max);
  MNERF_REQUIRE(dec->n_views >= 1 && dec->n_views * 4 < dec->cond_dim, MNERF_E_RANGE,
                "%s: n_views=%d inconsistent with cond_dim=%d", who, dec->n_views, dec->cond_dim);
  MNERF_REQUIRE(rays->n_rays >= 0 && rays->n_samples >= 1, MNERF_E_RANGE, "%s: n_rays=%d S=%d", who,
                rays->n_rays, rays->n_samples);
  const int Sp = pick_padded_samples(rays->n_samples);
  MNERF_REQUIRE(Sp > 0, MNERF_E_UNSUPPORTED, "%s: sample_intvs=%d > 256 is not supported by the fused kernel", who,
                rays->n_samples);
  if (rays->pose_table) {
    MNERF_REQUIRE(rays->rays_per_pose > 0 && rays->rays_per_pose % 64 == 0, MNERF_E_RANGE,
                  "%s: pose table needs rays_per_pose = a positive multiple of 64, got %d", who, rays->rays_per_pose);
    MNERF_REQUIRE(!rays->ray_idx && !rays->strat_u && !c.ext_ndc && !c.fused_scene, MNERF_E_UNSUPPORTED,
                  "%s: a pose table excludes ray_idx / strat_u / caller-supplied samples / the one-launch form", who);
  } else {
    MNERF_REQUIRE(rays->rays_per_pose == 0, MNERF_E_RANGE, "%s: rays_per_pose=%d without a pose table", who, rays->rays_per_pose);
  }
  const int total = build_schedule(dec, sch);
  MNERF_REQUIRE(total > 0, MNERF_E_RANGE, "%s: cannot schedule weight stream", who);
  MNERF_REQUIRE(dec->wstream_floats == total, MNERF_E_RANGE, "%s: wstream has %lld floats, schedule expects %d", who,
                (long long)dec->wstream_floats, total);
  *Sp_out = Sp;
  return MNERF_OK;
}
