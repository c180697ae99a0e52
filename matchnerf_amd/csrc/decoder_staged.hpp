// decoder_kernel<NW,SP,FMT,CVF>: the STAGED form of the ray-chunk kernel (decoder_common.hpp has the overview) and its launcher.
// fp32 data and accumulation; matrix products on the exact-f32 MFMA (FMT = 0), as fp32-grade products of three bf16 terms per
// operand on the bf16 MFMA (FMT = 1, "bf16x6") or of two fp16 terms per operand on the fp16 MFMA (FMT = 2, "f16x3", what the
// library packs by default).  Since round 3 the default decoder is the ping-pong kernel of decoder.hip; this kernel takes what that
// one does not: the f32 and bf16x6 streams, 6+ source views beyond 64 samples per ray, MNERF_DECODER_PP=0 - and, with CVF = 1, it
// is the one-launch form of the ray chunk (decoder_fused.hip).  Included by decoder.hip (CVF = 0) and decoder_fused.hip (CVF = 1).
//
// ---- MFMA formulation (the part that is specific to CDNA; described for FMT = 0) --------------
// Every Linear is evaluated TRANSPOSED:  Y^T[out, sample] = W[out, in] . H^T[in, sample]
// with v_mfma_f32_32x32x2_f32:  A = W tile (32 outs x 2 ins), B = H^T (2 ins x 32 samples).
// A wave owns 32 samples (N = lane&31) and all 128 outputs (4 M-blocks -> 4 x 16 accumulator
// VGPRs).  The C/D layout puts output row (r&3)+8*(r>>2)+4*(lane>>5) of block m in register
// r of lane (n, half) — which is exactly the B-operand layout the NEXT layer needs if its
// K-steps are taken in the order "register r of block m": lower half-wave supplies input
// feature f_lo(m,r), upper half supplies f_hi(m,r) = f_lo + 4.  Since a dot product does not
// care about the order of its terms, the host packs each weight matrix with its columns
// permuted to that order (matchnerf_amd/cond_nerf.py: pack_wstream, pack_wstream16), and the whole
// 6-layer MLP + heads chains accumulator -> operand with NO transpose, shuffle or LDS round trip.
// Biases ride along as one extra K-step whose B operand is the constant (1 | 0); the FiLM
// multiplier (pts_bias(cond), cond_nerf.py:62) is itself computed by an MFMA stage and kept
// in 64 VGPRs; the epilogue of a layer is one v_mul + v_max per accumulator register.
//
// Weights: 130k floats (521 KB as fp32 fragments, 808 KB as three bf16 terms) cannot live in LDS, so the packed A-fragment stream is cut
// into segments of <= 33 KiB that every wave consumes in the same order; segment i+1 is
// DMA'd global->LDS (global_load_lds_dwordx4, no VGPRs) into the other half of a double
// buffer while segment i feeds the MFMAs; one workgroup barrier per segment.
// With NW=4 a workgroup (a tile of TILE = 32*NW samples, whole rays) needs 76 KiB of LDS and <=256 VGPRs, so two workgroups share
// a CU (2 waves/SIMD) and de-synchronise: one's VALU phases (posenc, attention, compositing)
// overlap the other's MFMA phases.
#pragma once
#include "decoder_common.hpp"

template <int NW, int SP>
struct Smem {
  static constexpr int TILE = NW * 32;
  static constexpr int W_FLOATS = 2 * SEG_CAP_FLOATS;
  static constexpr int RS_FLOATS = TILE * 4;
  static constexpr int LN_FLOATS = 64;
  // Ray-attention scratch lives in the weight buffer that does NOT hold the resident tail segment.
  //   MFMA form (SP <= 128): K [rays][4][SP][4], V^T [rays][4][4][SP], Q [TILE][16], O [TILE][16]
  //   VALU form (SP  = 256): K|V interleaved [rays][4][SP][8]
  static constexpr bool MFMA_ATT = SP <= 128;
  static constexpr int KV_FLOATS = MFMA_ATT ? TILE * 64 : TILE * 32;
  static_assert(KV_FLOATS <= SEG_CAP_FLOATS, "attention scratch must fit one weight buffer");
  static constexpr int TOTAL_FLOATS = W_FLOATS + RS_FLOATS + LN_FLOATS;
};

// CVF = 1: the FUSED ray-chunk form (K1..K5 in one launch): the workgroup first produces the conditioning rows of
// its own tile with the register-quad walk of cv_walk.hpp (8-sample walks, one per 16-lane slot) straight into LDS
// — no [rays*S, cond_stride] hand-off through HBM — and only then starts the MFMA trunk.  The walk is texture /
// VALU work with no matrix instruction; with two workgroups per CU one workgroup's walk runs under the other's MFMA
// stages.  LDS: walk scratch in weight buffer 1, the tile's rows in the part of weight buffer 0 above segment 0
// (the FiLM weights: 17 KiB at <= 32 conditioning inputs); both are dead before the weight pipeline needs them.
#define CVF_SEG 8
#define CVF_COND_OFF_FLOATS (17 * 256)
// Two workgroups of the fused form share a CU like those of the staged decoder (68.25 KiB of LDS each).  Round 2 saw a
// handful of wrong rays per frame in that configuration and reserved the CU (84 KiB) without finding the cause.  Round 3
// found it (tools/exp/race_probe.py): the conditioning rows were wrong, always in lanes 48-63 of a
// wave, one walk step (or one pass-1 view) at a time — packed-fp32 vector instructions (v_pk_fma_f32 / v_pk_mul_f32) of
// the walk lose their result in the last lane quarter while ANOTHER wave of the SIMD issues v_mfma_f32_32x32x16_{f16,
// bf16}; the stand-alone cost volume shows the same faults when it runs next to this decoder on a second stream, not next
// to the exact-f32 decoder, and none once it is built without packed-fp32 instructions.  Both objects that hold this
// kernel are therefore compiled with -fno-slp-vectorize (build.py; the walk's own arithmetic is unpacked in cv_walk.hpp), and
// the occupancy restriction is gone: the kernel asks for its natural LDS footprint.
#define MNERF_DECODER_MINBLOCKS 2  // experiments: 1 = 512 registers per wave (one workgroup per CU), no spills
template <int NW, int SP, int FMT, int CVF>
__global__ __launch_bounds__(NW * 64, MNERF_DECODER_MINBLOCKS) void decoder_kernel(
    mnerf_decoder D, DecSched sch, mnerf_view view0, mnerf_rays R,
    const float* __restrict__ cond, float* __restrict__ out_rgb, float* __restrict__ out_depth,
    float* __restrict__ out_opacity, float* __restrict__ dbg_rgb_s, float* __restrict__ dbg_sigma,
    const float* __restrict__ ext_ndc, const float* __restrict__ ext_dir, mnerf_scene scene) {
  static_assert(!CVF || (FMT == 2 && NW == 4), "the fused form is built for the split-fp16 trunk");
  constexpr int Sp = SP;
  using SM = Smem<NW, SP>;
  constexpr int TILE = SM::TILE;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wbuf0 = smem;
  float* wbuf1 = smem + SEG_CAP_FLOATS;
  // LDS byte addresses of the two weight buffers, for the DMA and for the split-bf16 operand reads.  (No
  // generic->LDS pointer casts anywhere near the hot loops: they trip a gfx950 code-generation bug in hipcc
  // 7.2 — "Illegal instruction detected: Operand has incorrect register class" on a V_CMP against
  // src_shared_base — depending on unrelated code around them.)
  const unsigned wbuf0_lds = __builtin_amdgcn_groupstaticsize();  // the dynamic array starts after the static LDS
  const unsigned wbuf1_lds = wbuf0_lds + SEG_CAP_FLOATS * 4u;
  float* rs_lds = smem + SM::W_FLOATS;                // [TILE][4]   rgb.xyz, sigma.w
  float* ln_lds = rs_lds + SM::RS_FLOATS;             // LayerNorm weight[16] | bias[16]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform
  const int n = lane & 31, hl = lane >> 5;
  const int S = R.n_samples;
  const int rays_per_tile = TILE / Sp;
  const int n_tiles = (R.n_rays + rays_per_tile - 1) / rays_per_tile;
  const int L3 = 3 * D.L_3D;
  const int CS = D.cond_stride;
  const float freq_mul = R.legacy_coord ? 1.0f : 3.14159265358979323846f;
  const float wm1 = (float)(R.width - 1), hm1 = (float)(R.height - 1);

  // Phase stagger.  With <=256 VGPRs and 76 KiB of LDS two workgroups share a CU (one wave of
  // each per SIMD).  Launched together they run IN PHASE: their VALU-only phases (prologue,
  // ray attention, compositing) coincide and the matrix pipe idles for both (measured: MFMA busy
  // 69.6 % = 2M/(2M+V)).  The grid is persistent (2 workgroups per CU), and the workgroup whose
  // waves sit in the odd hardware wave slot waits half a tile ONCE, so that from then on one
  // workgroup's VALU phases overlap the other's MFMA phases.  Speed only: any placement is correct.
  if (sch.stagger_sleeps > 0) {
    const unsigned hw_id = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (3 << 11));  // HW_ID.WAVE_ID
    bool late = (hw_id & 1u) != 0;
    if (sch.stagger_mode == 1) late = blockIdx.x >= (gridDim.x >> 1);
    if (sch.stagger_mode == 2) late = ((blockIdx.x >> 3) & 1) != 0;
    if (sch.stagger_mode == 3) late = true;
    if (late)
      for (int i = 0; i < sch.stagger_sleeps; ++i) __builtin_amdgcn_s_sleep(127);
  }
  if (tid < SMALL_FIXED) ln_lds[tid] = D.small_[tid];
  __syncthreads();

  // Per-tile global inputs of a lane: its half-wave's FiLM operands (cond row) and the sum of the
  // visibility masks (cond_nerf.py:79-80).  (Fetching them one tile ahead was tried: the 33 extra
  // loop-carried VGPRs cost more in spills than the hidden latency gained.)
  float4 cpre[8];
  float n_valid = 0.0f;
  auto load_tile_inputs = [&](int t) {
    const int s_l = wave * 32 + n;
    const int r_t = s_l / Sp;
    const int j_p = s_l - r_t * Sp;
    int r = t * rays_per_tile + r_t;
    if (r >= R.n_rays) r = R.n_rays - 1;
    // row of this lane's sample: in the staged form a row of the [rays*S, CS] buffer in global memory, in the fused
    // form a row of the tile's [TILE, CS] block in LDS (written by this workgroup a moment ago)
    const float* crow_base = CVF ? (wbuf0 + CVF_COND_OFF_FLOATS) + (size_t)(r_t * Sp + (j_p < S ? j_p : (S - 1))) * CS
                                 : cond + ((size_t)r * S + (j_p < S ? j_p : (S - 1))) * CS;
    if constexpr (FMT >= 1) {  // K16 steps 0,1: cond[16 t + 8 hl + 4 q .. +4), q = i & 1, t = i >> 1
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * (i >> 1) + 8 * hl + 4 * (i & 1);
        cpre[i] = (o + 4 <= CS && (i >> 1) < sch.film_steps) ? ld_stream4(crow_base + o, CVF)
                                                            : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
      const float4* crow4 = reinterpret_cast<const float4*>(crow_base + (size_t)hl * sch.film_steps);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        cpre[i] = (4 * i < sch.film_steps) ? crow4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float* mrow = crow_base + (D.cond_dim - D.n_views);
    float nv = 0.0f;
    for (int v = 0; v < D.n_views; ++v) nv += mrow[v];
    n_valid = nv;
  };
  bool seg0_in_flight = false;

#ifdef MNERF_TIMELINE
  int tl_tile = -1;
  // record blocks [0,64) and their presumed CU partners [256,320)
  const int tl_slot = blockIdx.x < 64 ? (int)blockIdx.x : ((blockIdx.x >= 256 && blockIdx.x < 320) ? (int)blockIdx.x - 192 : -1);
#endif
  // Tile -> workgroup mapping.  Workgroup b runs on XCD b % 8 (observed dispatch order; speed only): XCD x takes the
  // contiguous tile range [x n/8, (x+1) n/8) and its workgroups step through it together, so the epipolar texels
  // the fused form gathers for concurrently processed tiles sit in that XCD's own L2.
  int tile_begin = blockIdx.x, tile_end = n_tiles, tile_step = gridDim.x;
  if (gridDim.x >= 8) {
    const int xcd = blockIdx.x & 7;
    tile_begin = (int)((long long)n_tiles * xcd / 8) + (int)(blockIdx.x >> 3);
    tile_end = (int)((long long)n_tiles * (xcd + 1) / 8);
    tile_step = ((int)gridDim.x - xcd + 7) >> 3;  // workgroups with this b % 8
  }
  for (int tile = tile_begin; tile < tile_end; tile += tile_step) {
#ifdef MNERF_TIMELINE
    ++tl_tile;
    if (sch.tl && lane == 0 && tl_slot >= 0 && tl_tile < 4)
      sch.tl[(((size_t)tl_slot * 4 + tl_tile) * NW + wave) * TL_POINTS + 19] =
          __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));  // HW_ID
#endif
    TL_STAMP(0);
#ifdef MNERF_TIMELINE
    unsigned long long tl_dma_wait = 0, tl_bar_wait = 0;
#endif
    // ------------------------------------------------------------ per-lane sample identity
    const int s_local = wave * 32 + n;
    const int ray_t = s_local / Sp;                 // ray within the tile
    const int jp = s_local - ray_t * Sp;            // padded sample slot
    const int ray_raw = tile * rays_per_tile + ray_t;
    const bool ray_ok = ray_raw < R.n_rays;
    const int ray = ray_ok ? ray_raw : (R.n_rays - 1);
    const int j = jp < S ? jp : (S - 1);            // padded slots recompute the last sample
    const size_t gs = (size_t)ray * S + j;          // global sample index

    float x, y, z, dx, dy, dz;
    if (ext_ndc) {
      // mnerf_decoder_samples: the caller supplies the decoder inputs of CondNeRF.forward (cond_nerf.py:52) —
      // sample coordinates w.r.t. source view 0 and the (already rotated) unit view direction per sample
      x = ext_ndc[gs * 3 + 0];
      y = ext_ndc[gs * 3 + 1];
      z = ext_ndc[gs * 3 + 2];
      dx = ext_dir[gs * 3 + 0];
      dy = ext_dir[gs * 3 + 1];
      dz = ext_dir[gs * 3 + 2];
    } else {
      const RayGeom g = make_ray(R, ray);
      const float dpt = sample_depth(R, ray, j);
      float wx_, wy_, wz_;
      ray_point(g, dpt, wx_, wy_, wz_);
      project(view0, wx_, wy_, wz_, wm1, hm1, x, y, z);
      // view direction in the frame of source view 0 (matchnerf.py:129-131)
      const float rn = fmaxf(sqrtf(g.rx * g.rx + g.ry * g.ry + g.rz * g.rz), 1e-12f);
      const float ux = g.rx / rn, uy = g.ry / rn, uz = g.rz / rn;
      dx = ux * view0.extr[0] + uy * view0.extr[1] + uz * view0.extr[2];
      dy = ux * view0.extr[4] + uy * view0.extr[5] + uz * view0.extr[6];
      dz = ux * view0.extr[8] + uy * view0.extr[9] + uz * view0.extr[10];
    }

    const EncBase encb = enc_base(x, y, z, freq_mul);  // shared by the two positional-encoding stages (L0, L5)
    int seg = 0;   // running segment index; segment k lives in buffer (k & 1)
#ifdef MNERF_FUSED_DEBUG
    const unsigned dflags = CVF ? sch.dbg_flags : 0u;
    if (CVF && sch.dbg_tile && tid == 0) {
      sch.dbg_tile[tile * 4 + 0] = blockIdx.x;
      sch.dbg_tile[tile * 4 + 1] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));   // HW_ID
      sch.dbg_tile[tile * 4 + 2] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));  // XCC_ID
      sch.dbg_tile[tile * 4 + 3] = (unsigned)__builtin_amdgcn_s_memtime();
    }
    if (!(dflags & 4u))
#endif
    if (!seg0_in_flight) prefetch_segment<NW>(D.wstream, sch, 0, wbuf0_lds, wave, lane);
#ifdef MNERF_FUSED_DEBUG
    if (dflags & 2u) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (dflags & 32u) {
      __syncthreads();
      for (int i = tid; i < SEG_CAP_FLOATS; i += NW * 64) wbuf1[i] = __builtin_nanf("");
      for (int i = CVF_COND_OFF_FLOATS + tid; i < SEG_CAP_FLOATS; i += NW * 64) wbuf0[i] = __builtin_nanf("");
      __syncthreads();
    }
#endif
    if constexpr (CVF) {
      // ---- K1+K2 for this tile: slot = 16 lanes, unit = CVF_SEG consecutive samples of one ray
      const int nv_ = scene.n_views;
      const int sumG_ = scene.n_group[0] + (scene.n_scales > 1 ? scene.n_group[1] : 0);
      const int per_slot = cv_slot_lds_floats(CVF_SEG, nv_, sumG_);
      const int slot = tid >> 4, sub = tid & 15;
      float* sl = wbuf1 + slot * per_slot;
      float* cond_lds = wbuf0 + CVF_COND_OFF_FLOATS;
      for (int unit = slot; unit < TILE / CVF_SEG; unit += NW * 4) {
        const int ls0 = unit * CVF_SEG;             // first local sample of the unit
        const int r_t = ls0 / Sp, jp0 = ls0 - r_t * Sp;
        const int rr = tile * rays_per_tile + r_t;
        const bool live = rr < R.n_rays;
        cv_walk_unit<8, CVF_SEG>(scene, R, live ? rr : R.n_rays - 1, live, jp0,
                                 cond_lds + (size_t)(r_t * Sp + (jp0 < S ? jp0 : S - 1)) * CS, CS, sl,
                                 reinterpret_cast<float4*>(sl + CVF_SEG * nv_ * 2), sl + CVF_SEG * (nv_ * 2 + 16), sub);
      }
      __syncthreads();  // the tile's rows are complete
    }
    load_tile_inputs(tile);  // issued before the geometry above is consumed: latency overlaps it
    const bool q_valid = n_valid > 1.0f;
#ifdef MNERF_FUSED_DEBUG
    if constexpr (CVF && FMT >= 1) {
      if (sch.dbg_rows && ray_ok && jp < S) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int o = 16 * (i >> 1) + 8 * hl + 4 * (i & 1);
          *reinterpret_cast<float4*>(sch.dbg_rows + gs * 32 + o) = cpre[i];
        }
        if (hl == 0) sch.dbg_nv[gs] = n_valid;
      }
      if (dflags & 8u) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
      }
      if (dflags & 4u) prefetch_segment<NW>(D.wstream, sch, 0, wbuf0_lds, wave, lane);
    }
#endif
    segment_wait();
    __syncthreads();  // publishes weight segment 0; in the fused form also: every lane holds its FiLM inputs, so
                      // weight buffer 1 (walk scratch) and the rows above segment 0 may be overwritten from here on

#define CUR_BUF ((seg & 1) ? wbuf1 : wbuf0)
#define NXT_BUF ((seg & 1) ? wbuf0 : wbuf1)
#define SEG_BEGIN() prefetch_segment<NW>(D.wstream, sch, seg + 1, (seg & 1) ? wbuf0_lds : wbuf1_lds, wave, lane)
#ifdef MNERF_TIMELINE
#define SEG_END()                                                  \
  do {                                                             \
    const unsigned long long t0_ = __builtin_amdgcn_s_memtime();   \
    segment_wait();                                                \
    const unsigned long long t1_ = __builtin_amdgcn_s_memtime();   \
    __syncthreads();                                               \
    const unsigned long long t2_ = __builtin_amdgcn_s_memtime();   \
    tl_dma_wait += t1_ - t0_;                                      \
    tl_bar_wait += t2_ - t1_;                                      \
    ++seg;                                                         \
  } while (0)
#else
#define SEG_END()     \
  do {                \
    segment_wait();   \
    __syncthreads();  \
    ++seg;            \
  } while (0)
#endif

    TL_STAMP(1);
    float av[8];  // alpha-head activations: rows 0..15 <-> registers 0..7, feature (r&3) + 8*(r>>2) + 4*hl
    if constexpr (FMT == 2) {
      // ============================================================ trunk, split-fp16 matrix path
      // Scale bookkeeping: register values carry an integer exponent per lane (the same in the two lanes of a
      // sample): true value = register * 2^ec.  A stage picks the operand gain 2^em from the sample's largest
      // operand, the accumulator then holds 2^(ew + em - ec) (W h_true + b), i.e. its exponent is ec - em - ew.
      unsigned wb;
#define CUR_LDS ((seg & 1) ? wbuf1_lds : wbuf0_lds)
      // ------------------------------------------------------------ FiLM = pts_bias(cond); inputs in [-1, 1]
      f32x16 film[4];
      int ecf = 0;  // film_true = film * 2^ecf (never multiplied out: it rides in the exponent of each layer)
      // (defined on every path before the segment loop: a value that is only assigned under `done == 0` inside the loop
      // looks possibly-undefined to the register allocator, which then keeps its 64 registers reserved from the top of
      // the tile loop - across the whole fused cost-volume phase)
#pragma unroll
      for (int m = 0; m < 4; ++m) film[m] = (f32x16)(0.0f);
      {
        int done = 0;
        while (done < sch.film_steps) {
          const int ns = sch.seg_steps[seg];
          SEG_BEGIN();
          wb = CUR_LDS;
          if (done == 0) {
            const int ew = header_ew(CUR_LDS);
            ecf = -(ew + (H16_TARGET_EXP - 1));
            bias_init_h<4>(film, CUR_LDS, hl, pow2i(ew + (H16_TARGET_EXP - 1)));
            wb += 1024;
          }
          for (int u = 0; u < ns; ++u) {
            const int t = done + u;
            float v[8];
            float4 c0, c1;
            if (t == 0) {
              c0 = cpre[0];
              c1 = cpre[1];
            } else if (t == 1) {
              c0 = cpre[2];
              c1 = cpre[3];
            } else {  // more than 32 conditioning inputs (n_src_views > 5): straight from global
              const int o = 16 * t + 8 * hl;
              const float* crow = cond + gs * CS;
              c0 = (o + 4 <= CS) ? *reinterpret_cast<const float4*>(crow + o) : make_float4(0.f, 0.f, 0.f, 0.f);
              c1 = (o + 8 <= CS) ? *reinterpret_cast<const float4*>(crow + o + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            v[0] = c0.x; v[1] = c0.y; v[2] = c0.z; v[3] = c0.w;
            v[4] = c1.x; v[5] = c1.y; v[6] = c1.z; v[7] = c1.w;
            ksteps_h<4, 1>(film, wb + u * 4 * H16_UNIT_BYTES, lane, v, (float)(1 << (H16_TARGET_EXP - 1)));
          }
          done += ns;
          SEG_END();
        }
      }
      TL_STAMP(2);
      // ------------------------------------------------------------ positional-encoding stages (L0, L5)
      f32x16 acc[4], h[4];
      const float enc_max = fmaxf(fmaxf(1.0f, fabsf(x)), fmaxf(fabsf(y), fabsf(z)));  // sin / cos <= 1; raw x, y, z
      int ew_cur = 0;
      // acc (+)= W_enc . enc(x) with operand gain 2^em; the first call of a stage loads bias * 2^(ew + em)
      auto enc_stage = [&](int em) {
        const float mult = pow2i(em);
        if (D.L_3D == 10) {  // one segment of four K16-steps, register-fed in two halves
          SEG_BEGIN();
          ew_cur = header_ew(CUR_LDS);
          bias_init_h<4>(acc, CUR_LDS, hl, pow2i(ew_cur + em));
          {
            const f32x16 e0 = enc_block16_L10<0>(encb, hl, x, y, z);
            kblock_h<4>(acc, CUR_LDS + 1024, lane, e0, mult);
          }
          {
            const f32x16 e1 = enc_block16_L10<16>(encb, hl, x, y, z);
            kblock_h<4>(acc, CUR_LDS + 1024 + 8 * H16_UNIT_BYTES, lane, e1, mult);
          }
          SEG_END();
        } else {
#pragma unroll
          for (int m = 0; m < 4; ++m) acc[m] = (f32x16)(0.0f);
          int done = 0;
          while (done < sch.enc_steps) {
            const int ns = sch.seg_steps[seg];
            SEG_BEGIN();
            wb = CUR_LDS;
            if (done == 0) {
              ew_cur = header_ew(CUR_LDS);
              bias_init_h<4>(acc, CUR_LDS, hl, pow2i(ew_cur + em));
              wb += 1024;
            }
            for (int u = 0; u < ns; ++u) {
              float v[8];
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = enc_operand(8 * (done + u) + j, L3, hl, x, y, z, freq_mul);
              ksteps_h<4, 1>(acc, wb + u * 4 * H16_UNIT_BYTES, lane, v, mult);
            }
            done += ns;
            SEG_END();
          }
        }
      };
      // acc (+)= W . h with register gain `mult`; with a header: acc <- bias * 2^bexp first (bexp - ew given)
      auto hidden_stage = [&](bool with_hdr, float mult, int bexp_minus_ew) {
#pragma unroll
        for (int sgi = 0; sgi < 2; ++sgi) {
          SEG_BEGIN();
          wb = CUR_LDS;
          if (sgi == 0 && with_hdr) {
            ew_cur = header_ew(CUR_LDS);
            bias_init_h<4>(acc, CUR_LDS, hl, pow2i(ew_cur + bexp_minus_ew));
            wb += 1024;
          }
          kblock_h<4>(acc, wb, lane, h[2 * sgi], mult);
          kblock_h<4>(acc, wb + 8 * H16_UNIT_BYTES, lane, h[2 * sgi + 1], mult);
          SEG_END();
        }
      };
      // h <- max(acc * film, 0); returns the sample's largest new activation (register units)
      auto film_relu = [&]() -> float {
        float mx = 0.0f;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float t = fmaxf(acc[m][r] * film[m][r], 0.0f);
            h[m][r] = t;
            mx = fmaxf(mx, t);
          }
        return fmaxf(mx, __shfl_xor(mx, 32, 64));
      };
      int ec;  // exponent of the values in h
      {
        const int em = gain_exp(enc_max);
        enc_stage(em);
        ec = -em - ew_cur + ecf;
      }
      float hmax = film_relu();
      TL_STAMP(3);
      // ------------------------------------------------------------ layers 1..4: 128 -> 128
      for (int layer = 1; layer <= 4; ++layer) {
        const int em = gain_exp(hmax);
        hidden_stage(true, pow2i(em), em - ec);
        ec = ec - em - ew_cur + ecf;
        hmax = film_relu();
      }
      TL_STAMP(4);
      // ------------------------------------------------------------ layer 5: [enc, h] -> 128, one accumulator:
      // both operand sets share one TRUE gain 2^eg, from the larger of the two maxima
      {
        const int eg = gain_exp(fmaxf(enc_max, hmax * pow2i(ec)));
        enc_stage(eg);
        hidden_stage(false, pow2i(eg + ec), 0);
        ec = -eg - ew_cur + ecf;
        hmax = film_relu();
      }
      // ------------------------------------------------------------ alpha head: 128 -> 16 (its activations wait in 8 registers for the ray transformer)
      const int em5 = gain_exp(hmax);
      const float mult5 = pow2i(em5);
      {
        f32x16 al[1];
        SEG_BEGIN();
        wb = CUR_LDS + 1024;
        const int ew = header_ew(CUR_LDS);
        bias_init_h<1>(al, CUR_LDS, hl, pow2i(ew + em5 - ec));
        const float ca = pow2i(ec - em5 - ew);
#pragma unroll
        for (int sgi = 0; sgi < 4; ++sgi) kblock_h<1>(al, wb + sgi * 2 * H16_UNIT_BYTES, lane, h[sgi], mult5);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          float t = al[0][r] * ca;
          t = D.raytrans_elu ? (t > 0.0f ? t : (expf(t) - 1.0f)) : fmaxf(t, 0.0f);
          av[r] = t;
        }
        if (D.raytrans_posenc) {
          const float* tab = D.small_ + SMALL_FIXED + (size_t)j * 16;
#pragma unroll
          for (int r = 0; r < 8; ++r) av[r] += tab[(r & 3) + 8 * (r >> 2) + 4 * hl];
        }
        SEG_END();
      }
      TL_STAMP(5);
      // ------------------------------------------------------------ feature_linear: 128 -> 128 (no activation)
      hidden_stage(true, mult5, em5 - ec);
      const int ecfeat = ec - em5 - ew_cur;
      TL_STAMP(6);
      // ------------------------------------------------------------ views_linear: [feat, dir] -> 64
      f32x16 hv[2];
      int ecv;
      {
        const int eg = gain_exp(fmaxf(1.0f, sample_absmax<4>(acc) * pow2i(ecfeat)));  // |dir| <= 1
        const float multf = pow2i(eg + ecfeat), multd = pow2i(eg);
        SEG_BEGIN();
        wb = CUR_LDS + 1024;
        const int ew = header_ew(CUR_LDS);
        bias_init_h<2>(hv, CUR_LDS, hl, pow2i(ew + eg));
        kblock_h<2>(hv, wb, lane, acc[0], multf);
        kblock_h<2>(hv, wb + 4 * H16_UNIT_BYTES, lane, acc[1], multf);
        SEG_END();
        SEG_BEGIN();
        wb = CUR_LDS;
        kblock_h<2>(hv, wb, lane, acc[2], multf);
        kblock_h<2>(hv, wb + 4 * H16_UNIT_BYTES, lane, acc[3], multf);
        const float v[8] = {hl ? 0.0f : dx, hl ? 0.0f : dy, hl ? 0.0f : dz, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        ksteps_h<2, 1>(hv, wb + 8 * H16_UNIT_BYTES, lane, v, multd);
        SEG_END();
        ecv = -eg - ew;
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) hv[m][r] = fmaxf(hv[m][r], 0.0f);
      TL_STAMP(7);
      // ------------------------------------------------------------ rgb_linear: 64 -> 3, sigmoid
      {
        const int em = gain_exp(sample_absmax<2>(hv));
        const float mult = pow2i(em);
        f32x16 c3[1];
        SEG_BEGIN();
        wb = CUR_LDS + 1024;
        const int ew = header_ew(CUR_LDS);
        bias_init_h<1>(c3, CUR_LDS, hl, pow2i(ew + em - ecv));
        const float cc = pow2i(ecv - em - ew);
        kblock_h<1>(c3, wb, lane, hv[0], mult);
        kblock_h<1>(c3, wb + 2 * H16_UNIT_BYTES, lane, hv[1], mult);
        if (hl == 0) {
          const float cr = 1.0f / (1.0f + expf(-c3[0][0] * cc));
          const float cg = 1.0f / (1.0f + expf(-c3[0][1] * cc));
          const float cb = 1.0f / (1.0f + expf(-c3[0][2] * cc));
          rs_lds[s_local * 4 + 0] = cr;
          rs_lds[s_local * 4 + 1] = cg;
          rs_lds[s_local * 4 + 2] = cb;
          if (dbg_rgb_s && ray_ok && jp < S) {
            dbg_rgb_s[gs * 3 + 0] = cr;
            dbg_rgb_s[gs * 3 + 1] = cg;
            dbg_rgb_s[gs * 3 + 2] = cb;
          }
        }
        SEG_END();
      }
      TL_STAMP(8);
#undef CUR_LDS
    } else if constexpr (FMT == 1) {
      // ============================================================ trunk, split-bf16 matrix path
      unsigned wb;  // LDS byte cursor inside the current weight segment
#define CUR_LDS ((seg & 1) ? wbuf1_lds : wbuf0_lds)
      // ------------------------------------------------------------ FiLM = pts_bias(cond)
      f32x16 film[4];
      {
        int done = 0;
        while (done < sch.film_steps) {
          const int ns = sch.seg_steps[seg];
          SEG_BEGIN();
          wb = CUR_LDS;
          if (done == 0) {
            bias_init<4>(film, CUR_LDS, hl);
            wb += 1024;
          }
          for (int u = 0; u < ns; ++u) {
            const int t = done + u;
            float v[8];
            float4 c0, c1;
            if (t == 0) {
              c0 = cpre[0];
              c1 = cpre[1];
            } else if (t == 1) {
              c0 = cpre[2];
              c1 = cpre[3];
            } else {  // more than 32 conditioning inputs (n_src_views > 5): straight from global
              const int o = 16 * t + 8 * hl;
              const float* crow = cond + gs * CS;
              c0 = (o + 4 <= CS) ? *reinterpret_cast<const float4*>(crow + o) : make_float4(0.f, 0.f, 0.f, 0.f);
              c1 = (o + 8 <= CS) ? *reinterpret_cast<const float4*>(crow + o + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            v[0] = c0.x; v[1] = c0.y; v[2] = c0.z; v[3] = c0.w;
            v[4] = c1.x; v[5] = c1.y; v[6] = c1.z; v[7] = c1.w;
            ksteps<4, 1>(film, wb + u * 4 * K16_UNIT_BYTES, lane, v);
          }
          done += ns;
          SEG_END();
        }
      }
      TL_STAMP(2);
      // ------------------------------------------------------------ positional-encoding stages (L0, L5)
      f32x16 acc[4], h[4];
      auto enc_stage = [&]() {  // acc <- bias + W_enc . enc(x)
        if (D.L_3D == 10) {  // two segments of two K16-steps, register-fed
          {
            const f32x16 e0 = enc_block16_L10<0>(encb, hl, x, y, z);
            SEG_BEGIN();
            bias_init<4>(acc, CUR_LDS, hl);
            kblock<4>(acc, CUR_LDS + 1024, lane, e0);
            SEG_END();
          }
          {
            const f32x16 e1 = enc_block16_L10<16>(encb, hl, x, y, z);
            SEG_BEGIN();
            kblock<4>(acc, CUR_LDS, lane, e1);
            SEG_END();
          }
        } else {
          int done = 0;
          while (done < sch.enc_steps) {
            const int ns = sch.seg_steps[seg];
            SEG_BEGIN();
            wb = CUR_LDS;
            if (done == 0) {
              bias_init<4>(acc, CUR_LDS, hl);
              wb += 1024;
            }
            for (int u = 0; u < ns; ++u) {
              float v[8];
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = enc_operand(8 * (done + u) + j, L3, hl, x, y, z, freq_mul);
              ksteps<4, 1>(acc, wb + u * 4 * K16_UNIT_BYTES, lane, v);
            }
            done += ns;
            SEG_END();
          }
        }
      };
      auto hidden_stage = [&](bool with_bias) {  // acc (+)= W . h : four segments, one per input block
#pragma unroll
        for (int sgi = 0; sgi < 4; ++sgi) {
          SEG_BEGIN();
          wb = CUR_LDS;
          if (sgi == 0 && with_bias) {
            bias_init<4>(acc, CUR_LDS, hl);
            wb += 1024;
          }
          kblock<4>(acc, wb, lane, h[sgi]);
          SEG_END();
        }
      };
      enc_stage();
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) h[m][r] = fmaxf(acc[m][r] * film[m][r], 0.0f);
      TL_STAMP(3);
      // ------------------------------------------------------------ layers 1..4: 128 -> 128
      for (int layer = 1; layer <= 4; ++layer) {
        hidden_stage(true);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 16; ++r) h[m][r] = fmaxf(acc[m][r] * film[m][r], 0.0f);
      }
      TL_STAMP(4);
      // ------------------------------------------------------------ layer 5: [enc, h] -> 128
      enc_stage();
      hidden_stage(false);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) h[m][r] = fmaxf(acc[m][r] * film[m][r], 0.0f);
      // ------------------------------------------------------------ alpha head: 128 -> 16 (its activations wait in 8 registers for the ray transformer)
      {
        f32x16 al[1];
        SEG_BEGIN();
        wb = CUR_LDS + 1024;
        bias_init<1>(al, CUR_LDS, hl);
#pragma unroll
        for (int sgi = 0; sgi < 4; ++sgi) kblock<1>(al, wb + sgi * 2 * K16_UNIT_BYTES, lane, h[sgi]);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          float t = al[0][r];
          t = D.raytrans_elu ? (t > 0.0f ? t : (expf(t) - 1.0f)) : fmaxf(t, 0.0f);
          av[r] = t;
        }
        if (D.raytrans_posenc) {
          const float* tab = D.small_ + SMALL_FIXED + (size_t)j * 16;
#pragma unroll
          for (int r = 0; r < 8; ++r) av[r] += tab[(r & 3) + 8 * (r >> 2) + 4 * hl];
        }
        SEG_END();
      }
      TL_STAMP(5);
      // ------------------------------------------------------------ feature_linear: 128 -> 128
      hidden_stage(true);
      TL_STAMP(6);
      // ------------------------------------------------------------ views_linear: [feat, dir] -> 64
      f32x16 hv[2];
      {
        SEG_BEGIN();
        wb = CUR_LDS + 1024;
        bias_init<2>(hv, CUR_LDS, hl);
        kblock<2>(hv, wb, lane, acc[0]);
        kblock<2>(hv, wb + 4 * K16_UNIT_BYTES, lane, acc[1]);
        SEG_END();
        SEG_BEGIN();
        wb = CUR_LDS;
        kblock<2>(hv, wb, lane, acc[2]);
        kblock<2>(hv, wb + 4 * K16_UNIT_BYTES, lane, acc[3]);
        const float v[8] = {hl ? 0.0f : dx, hl ? 0.0f : dy, hl ? 0.0f : dz, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        ksteps<2, 1>(hv, wb + 8 * K16_UNIT_BYTES, lane, v);
        SEG_END();
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) hv[m][r] = fmaxf(hv[m][r], 0.0f);
      TL_STAMP(7);
      // ------------------------------------------------------------ rgb_linear: 64 -> 3, sigmoid
      {
        f32x16 c3[1];
        SEG_BEGIN();
        wb = CUR_LDS + 1024;
        bias_init<1>(c3, CUR_LDS, hl);
        kblock<1>(c3, wb, lane, hv[0]);
        kblock<1>(c3, wb + 2 * K16_UNIT_BYTES, lane, hv[1]);
        if (hl == 0) {
          const float cr = 1.0f / (1.0f + expf(-c3[0][0]));
          const float cg = 1.0f / (1.0f + expf(-c3[0][1]));
          const float cb = 1.0f / (1.0f + expf(-c3[0][2]));
          rs_lds[s_local * 4 + 0] = cr;
          rs_lds[s_local * 4 + 1] = cg;
          rs_lds[s_local * 4 + 2] = cb;
          if (dbg_rgb_s && ray_ok && jp < S) {
            dbg_rgb_s[gs * 3 + 0] = cr;
            dbg_rgb_s[gs * 3 + 1] = cg;
            dbg_rgb_s[gs * 3 + 2] = cb;
          }
        }
        SEG_END();
      }
      TL_STAMP(8);
#undef CUR_LDS
    } else {
      // ============================================================ trunk, exact-f32 MFMA path
    // ------------------------------------------------------------ FiLM = pts_bias(cond)
    f32x16 film[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) film[m] = (f32x16)(0.0f);
    {
      // cond_stride <= 64 => film_steps <= 32 => one segment; inputs preloaded in cpre[]
      const int ns = sch.seg_steps[seg];
      SEG_BEGIN();
      const float* wseg = CUR_BUF;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (4 * i < ns) {
          step4(film, wseg, 4 * i + 0, lane, cpre[i].x);
          step4(film, wseg, 4 * i + 1, lane, cpre[i].y);
          step4(film, wseg, 4 * i + 2, lane, cpre[i].z);
          step4(film, wseg, 4 * i + 3, lane, cpre[i].w);
        }
      }
      SEG_END();
    }

    TL_STAMP(2);
    // ------------------------------------------------------------ layer 0: enc -> 128
    f32x16 acc[4], h[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = (f32x16)(0.0f);
    if (D.L_3D == 10) {  // every shipped config: one segment, register-fed
      const f32x16 e0 = enc_block16_L10<0>(encb, hl, x, y, z);
      const f32x16 e1 = enc_block16_L10<16>(encb, hl, x, y, z);
      SEG_BEGIN();
      steps_from_regs<4>(acc, CUR_BUF, 0, lane, e0, e1);
      SEG_END();
    } else {
      int done = 0;
      while (done < sch.enc_steps) {
        const int ns = sch.seg_steps[seg];
        SEG_BEGIN();
        const float* wseg = CUR_BUF;
        for (int t = 0; t < ns; ++t)
          step4(acc, wseg, t, lane, enc_operand(done + t, L3, hl, x, y, z, freq_mul));
        done += ns;
        SEG_END();
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) h[m][r] = fmaxf(acc[m][r] * film[m][r], 0.0f);

    TL_STAMP(3);
    // ------------------------------------------------------------ layers 1..4: 128 -> 128
    for (int layer = 1; layer <= 4; ++layer) {
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = (f32x16)(0.0f);
      SEG_BEGIN();
      steps_from_regs<4>(acc, CUR_BUF, 0, lane, h[0], h[1]);
      SEG_END();
      SEG_BEGIN();
      steps_from_regs<4>(acc, CUR_BUF, 0, lane, h[2], h[3]);
      step4(acc, CUR_BUF, 32, lane, hl ? 0.0f : 1.0f);  // bias column
      SEG_END();
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) h[m][r] = fmaxf(acc[m][r] * film[m][r], 0.0f);
    }

    TL_STAMP(4);
    // ------------------------------------------------------------ layer 5: [enc, h] -> 128
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = (f32x16)(0.0f);
    if (D.L_3D == 10) {  // register-fed in two halves of 16 (film + h + acc are live here)
      SEG_BEGIN();
      {
        const f32x16 e = enc_block16_L10<0>(encb, hl, x, y, z);
        steps16_from_regs(acc, CUR_BUF, 0, lane, e);
      }
      {
        const f32x16 e = enc_block16_L10<16>(encb, hl, x, y, z);
        steps16_from_regs(acc, CUR_BUF, 16, lane, e);
      }
      SEG_END();
    } else {
      int done = 0;
      while (done < sch.enc_steps) {
        const int ns = sch.seg_steps[seg];
        SEG_BEGIN();
        const float* wseg = CUR_BUF;
        for (int t = 0; t < ns; ++t)
          step4(acc, wseg, t, lane, enc_operand(done + t, L3, hl, x, y, z, freq_mul));
        done += ns;
        SEG_END();
      }
    }
    SEG_BEGIN();
    steps_from_regs<4>(acc, CUR_BUF, 0, lane, h[0], h[1]);
    SEG_END();
    SEG_BEGIN();
    steps_from_regs<4>(acc, CUR_BUF, 0, lane, h[2], h[3]);
    SEG_END();
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) h[m][r] = fmaxf(acc[m][r] * film[m][r], 0.0f);

    TL_STAMP(5);
    // ------------------------------------------------------------ feature_linear: 128 -> 128
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = (f32x16)(0.0f);
    SEG_BEGIN();
    steps_from_regs<4>(acc, CUR_BUF, 0, lane, h[0], h[1]);
    SEG_END();
    SEG_BEGIN();
    steps_from_regs<4>(acc, CUR_BUF, 0, lane, h[2], h[3]);
    step4(acc, CUR_BUF, 32, lane, hl ? 0.0f : 1.0f);
    SEG_END();

    TL_STAMP(6);
    // ------------------------------------------------------------ views_linear: [feat, dir] -> 64
    f32x16 hv[2];
    hv[0] = (f32x16)(0.0f);
    hv[1] = (f32x16)(0.0f);
    {
      SEG_BEGIN();
      const float* wseg = CUR_BUF;
      steps_from_regs<2>(hv, wseg, 0, lane, acc[0], acc[1]);
      steps_from_regs<2>(hv, wseg, 32, lane, acc[2], acc[3]);
      step2(hv, wseg, 64, lane, hl ? dy : dx);
      step2(hv, wseg, 65, lane, hl ? 1.0f : dz);
      SEG_END();
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) hv[m][r] = fmaxf(hv[m][r], 0.0f);

    TL_STAMP(7);
    // ------------------------------------------------------------ rgb_linear: 64 -> 3, sigmoid
    {
      f32x16 c3[1];
      c3[0] = (f32x16)(0.0f);
      SEG_BEGIN();
      const float* wseg = CUR_BUF;
      steps_from_regs<1>(c3, wseg, 0, lane, hv[0], hv[1]);
      step1(c3[0], wseg, 32, lane, hl ? 0.0f : 1.0f);
      if (hl == 0) {
        const float cr = 1.0f / (1.0f + expf(-c3[0][0]));
        const float cg = 1.0f / (1.0f + expf(-c3[0][1]));
        const float cb = 1.0f / (1.0f + expf(-c3[0][2]));
        rs_lds[s_local * 4 + 0] = cr;
        rs_lds[s_local * 4 + 1] = cg;
        rs_lds[s_local * 4 + 2] = cb;
        if (dbg_rgb_s && ray_ok && jp < S) {
          dbg_rgb_s[gs * 3 + 0] = cr;
          dbg_rgb_s[gs * 3 + 1] = cg;
          dbg_rgb_s[gs * 3 + 2] = cb;
        }
      }
      SEG_END();
    }

    TL_STAMP(8);
    // ------------------------------------------------------------ alpha head: 128 -> 16 (last trunk stage:
    // its activations stay in registers and feed the ray transformer's MFMA stages directly)
    // rows 0..15 <-> registers 0..7: feature o = (r&3) + 8*(r>>2) + 4*hl
    {
      f32x16 al[1];
      al[0] = (f32x16)(0.0f);
      SEG_BEGIN();  // DMA of the tail segment
      const float* wseg = CUR_BUF;
      steps_from_regs<1>(al, wseg, 0, lane, h[0], h[1]);
      steps_from_regs<1>(al, wseg, 32, lane, h[2], h[3]);
      step1(al[0], wseg, 64, lane, hl ? 0.0f : 1.0f);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float t = al[0][r];
        t = D.raytrans_elu ? (t > 0.0f ? t : (expf(t) - 1.0f)) : fmaxf(t, 0.0f);
        av[r] = t;
      }
      if (D.raytrans_posenc) {
        const float* tab = D.small_ + SMALL_FIXED + (size_t)j * 16;
#pragma unroll
        for (int r = 0; r < 8; ++r) av[r] += tab[(r & 3) + 8 * (r >> 2) + 4 * hl];
      }
      SEG_END();
    }

    }

    // ============================================================ ray transformer (K4)
    // The tail segment [w_qs;w_ks;w_vs | fc | out_alpha.0 | out_alpha.2] stays resident in its
    // weight buffer; the OTHER buffer (last read before the barrier above) is the K/V/Q/O scratch.
    TL_STAMP(17);
    const float* tail = CUR_BUF;
    float* att = NXT_BUF;
#undef CUR_BUF
#undef NXT_BUF
#undef SEG_BEGIN
#undef SEG_END
    float* kv_lds = att;                // VALU form: [rays][4 heads][Sp][8] (k0..3, v0..3)
    float* k_lds = att;                 // MFMA form
    float* vt_lds = att + TILE * 16;
    float* q_lds = att + TILE * 32;
    float* o_lds = att + TILE * 48;
    (void)kv_lds; (void)k_lds; (void)vt_lds; (void)q_lds; (void)o_lds;

    // ---- q|k|v = [Wq;Wk;Wv] a : 8 K-steps x 2 M-blocks, operands straight from the alpha registers.
    // Result rows: block 0 = q (regs 0..7) | k (regs 8..15), block 1 = v (regs 0..7); this lane
    // holds heads {hl, 2+hl} of its sample (register quad hh <-> head hl + 2*hh).
    f32x16 qkv[2];
    qkv[0] = (f32x16)(0.0f);
    qkv[1] = (f32x16)(0.0f);
#pragma unroll
    for (int r = 0; r < 8; ++r) step2(qkv, tail + TAIL_QKV, r, lane, av[r]);
    TL_STAMP(18);
    // temperature sqrt(d_k) = 2; masked query row -> uniform.  The MFMA form keeps its scores in the log2 domain
    // (log2 e folded into the query scale): the softmax numerator is then one v_exp_f32 per key
    const float qs = q_valid ? (SM::MFMA_ATT ? 0.5f * 1.4426950408889634f : 0.5f) : 0.0f;

    float ofc[8];  // attention output features [8*hl, 8*hl+8) of this lane's sample (head-major)
    if constexpr (SM::MFMA_ATT) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int head = hl + 2 * hh;
        *reinterpret_cast<float4*>(k_lds + ((ray_t * 4 + head) * Sp + jp) * 4) =
            make_float4(qkv[0][8 + 4 * hh], qkv[0][9 + 4 * hh], qkv[0][10 + 4 * hh], qkv[0][11 + 4 * hh]);
        float* vcol = vt_lds + (ray_t * 4 + head) * 4 * Sp + jp;
        vcol[0] = qkv[1][4 * hh];
        vcol[Sp] = qkv[1][4 * hh + 1];
        vcol[2 * Sp] = qkv[1][4 * hh + 2];
        vcol[3 * Sp] = qkv[1][4 * hh + 3];
        *reinterpret_cast<float4*>(q_lds + s_local * 16 + head * 4) =
            make_float4(qkv[0][4 * hh] * qs, qkv[0][4 * hh + 1] * qs, qkv[0][4 * hh + 2] * qs, qkv[0][4 * hh + 3] * qs);
      }
      __syncthreads();
      TL_STAMP(9);
      TL_STAMP(10);
      // ---- attention proper on the matrix pipe: lane = query.  v_mfma_f32_4x4x1_16b runs 16
      // independent 4x4 outer products per instruction, D[r](lane) += A(lane 4*(l/4)+r) B(lane):
      //   scores of 4 keys  s4[r] += K[k0+r][d] * Q[query][d]     (A = K row l%4, 4 steps over d)
      //   output            o4[d] += V[key][d] * P[query][key]    (A = V^T row l%4, 1 step per key)
      // Scores / probabilities of all S keys stay in VGPRs (the MLP's registers are dead here).
      int a_ray, a_hp, a_jq;
      if constexpr (SP >= 64) {
        constexpr int CH = SP / 64;
        int idx = wave;
        const int chunk = idx % CH;
        idx /= CH;
        a_hp = idx & 1;
        a_ray = idx >> 1;
        a_jq = chunk * 64 + lane;
      } else {
        a_ray = wave;  // SP == 32: one ray per wave, the two head pairs in the two half-waves
        a_hp = lane >> 5;
        a_jq = lane & 31;
      }
      const int s_q = a_ray * Sp + a_jq;
      // the scores of one head take SP registers per lane: at SP = 128 the two heads must not be unrolled into one
      // schedule (their score sets would be live together: 300 spilled VGPRs)
      constexpr int HEAD_UNROLL = SP >= 128 ? 1 : 2;
#pragma unroll HEAD_UNROLL
      for (int hh = 0; hh < 2; ++hh) {
        const int head = 2 * a_hp + hh;
        const float4 q4 = *reinterpret_cast<const float4*>(q_lds + s_q * 16 + head * 4);
        const float* kb = k_lds + ((a_ray * 4 + head) * Sp + (lane & 3)) * 4;
        f32x4 sc[SP / 4];
#pragma unroll
        for (int g = 0; g < SP / 4; ++g) {
          const float4 kk = *reinterpret_cast<const float4*>(kb + g * 16);
          f32x4 t = {0.f, 0.f, 0.f, 0.f};
          t = mfma4(kk.x, q4.x, t);
          t = mfma4(kk.y, q4.y, t);
          t = mfma4(kk.z, q4.z, t);
          t = mfma4(kk.w, q4.w, t);
          sc[g] = t;
        }
        // four independent partial maxima / sums instead of one 64-long dependent chain
        float mx4[4] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
        if (S == Sp) {  // no padded key slots (the usual case): no per-key masks (SP run-time comparisons otherwise)
#pragma unroll
          for (int g = 0; g < SP / 4; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx4[r] = fmaxf(mx4[r], sc[g][r]);
        } else {
          // (an opaque copy of S: otherwise the SP comparisons are hoisted out of the tile loop as SP lane masks in
          // 2 SP scalar registers - spilled, and paid for by the unpadded case too)
          int s_keys = S;
          asm volatile("" : "+s"(s_keys));
#pragma unroll
          for (int g = 0; g < SP / 4; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float v = (4 * g + r < s_keys) ? sc[g][r] : -3.0e38f;  // padded key slots
              sc[g][r] = v;
              mx4[r] = fmaxf(mx4[r], v);
            }
        }
        const float mx = fmaxf(fmaxf(mx4[0], mx4[1]), fmaxf(mx4[2], mx4[3]));
        float ls4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < SP / 4; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pr = __builtin_amdgcn_exp2f(sc[g][r] - mx);
            sc[g][r] = pr;
            ls4[r] += pr;
          }
        const float lsum = (ls4[0] + ls4[1]) + (ls4[2] + ls4[3]);
        const float* vb = vt_lds + ((a_ray * 4 + head) * 4 + (lane & 3)) * Sp;
        f32x4 oa = {0.f, 0.f, 0.f, 0.f}, ob = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < SP / 4; g += 2) {
          const float4 va = *reinterpret_cast<const float4*>(vb + 4 * g);
          const float4 vc = *reinterpret_cast<const float4*>(vb + 4 * g + 4);
          oa = mfma4(va.x, sc[g][0], oa);
          ob = mfma4(vc.x, sc[g + 1][0], ob);
          oa = mfma4(va.y, sc[g][1], oa);
          ob = mfma4(vc.y, sc[g + 1][1], ob);
          oa = mfma4(va.z, sc[g][2], oa);
          ob = mfma4(vc.z, sc[g + 1][2], ob);
          oa = mfma4(va.w, sc[g][3], oa);
          ob = mfma4(vc.w, sc[g + 1][3], ob);
        }
        const float il = 1.0f / lsum;
        *reinterpret_cast<float4*>(o_lds + s_q * 16 + head * 4) =
            make_float4((oa[0] + ob[0]) * il, (oa[1] + ob[1]) * il, (oa[2] + ob[2]) * il, (oa[3] + ob[3]) * il);
      }
      __syncthreads();
      {
        const float4* src = reinterpret_cast<const float4*>(o_lds + s_local * 16 + 8 * hl);
        const float4 t0 = src[0], t1 = src[1];
        ofc[0] = t0.x; ofc[1] = t0.y; ofc[2] = t0.z; ofc[3] = t0.w;
        ofc[4] = t1.x; ofc[5] = t1.y; ofc[6] = t1.z; ofc[7] = t1.w;
      }
    } else {
      // ---- VALU form (S > 128): two lanes per sample, heads {hl, 2+hl}, K/V broadcast from LDS
      float ov[8];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        float4* dst = reinterpret_cast<float4*>(kv_lds + ((size_t)(ray_t * 4 + hl + 2 * hh) * Sp + jp) * 8);
        dst[0] = make_float4(qkv[0][8 + 4 * hh], qkv[0][9 + 4 * hh], qkv[0][10 + 4 * hh], qkv[0][11 + 4 * hh]);
        dst[1] = make_float4(qkv[1][4 * hh], qkv[1][4 * hh + 1], qkv[1][4 * hh + 2], qkv[1][4 * hh + 3]);
      }
      __syncthreads();
      TL_STAMP(9);
      TL_STAMP(10);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const float4* base = reinterpret_cast<const float4*>(kv_lds + (size_t)(ray_t * 4 + hl + 2 * hh) * Sp * 8);
        const float q0 = qkv[0][4 * hh] * qs, q1 = qkv[0][4 * hh + 1] * qs, q2 = qkv[0][4 * hh + 2] * qs,
                    q3 = qkv[0][4 * hh + 3] * qs;
        float mx = -3.0e38f;
        for (int jj = 0; jj < S; ++jj) {
          const float4 k4 = base[jj * 2];
          mx = fmaxf(mx, q0 * k4.x + q1 * k4.y + q2 * k4.z + q3 * k4.w);
        }
        float l = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
        for (int jj = 0; jj < S; ++jj) {
          const float4 k4 = base[jj * 2], v4 = base[jj * 2 + 1];
          const float p = __expf((q0 * k4.x + q1 * k4.y + q2 * k4.z + q3 * k4.w) - mx);
          l += p;
          o0 += p * v4.x;
          o1 += p * v4.y;
          o2 += p * v4.z;
          o3 += p * v4.w;
        }
        const float il = 1.0f / l;
        ov[hh * 4] = o0 * il;
        ov[hh * 4 + 1] = o1 * il;
        ov[hh * 4 + 2] = o2 * il;
        ov[hh * 4 + 3] = o3 * il;
      }
      // this lane has heads {hl, 2+hl}; the fc stage wants features [8 hl, 8 hl + 8) = heads {2hl, 2hl+1}
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const float mine_lo = ov[d], mine_hi = ov[4 + d];
        const float oth_lo = __shfl_xor(mine_lo, 32, 64), oth_hi = __shfl_xor(mine_hi, 32, 64);
        // hl = 0: heads 0 (mine_lo), 1 (partner's lo);  hl = 1: heads 2 (partner's hi), 3 (mine_hi)
        ofc[d] = hl ? oth_hi : mine_lo;
        ofc[4 + d] = hl ? mine_hi : oth_lo;
      }
    }

    TL_STAMP(11);
    // ---- fc (16x16, no bias) as one more MFMA stage + residual + LayerNorm(eps 1e-6); the 16
    // features of a sample are split over its two lanes exactly like the alpha registers.
    float yv[8];
    {
      f32x16 t1 = (f32x16)(0.0f);
#pragma unroll
      for (int t = 0; t < 8; ++t) step1(t1, tail + TAIL_FCO, t, lane, ofc[t]);
      float xs = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        yv[r] = t1[r] + av[r];
        xs += yv[r];
      }
      xs += __shfl_xor(xs, 32, 64);
      const float mean = xs * (1.0f / 16.0f);
      float var = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float dlt = yv[r] - mean;
        var += dlt * dlt;
      }
      var += __shfl_xor(var, 32, 64);
      const float rstd = 1.0f / sqrtf(var * (1.0f / 16.0f) + 1e-6f);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int o = (r & 3) + 8 * (r >> 2) + 4 * hl;
        yv[r] = (yv[r] - mean) * rstd * ln_lds[o] + ln_lds[16 + o];
      }
    }
    // ---- out_alpha_linear: 16 -> 16 (act) -> 1 (ReLU) as two MFMA stages (cond_nerf.py:33-36, 84)
    float sigma;
    {
      f32x16 t2 = (f32x16)(0.0f);
#pragma unroll
      for (int r = 0; r < 8; ++r) step1(t2, tail + TAIL_OA0, r, lane, yv[r]);
      step1(t2, tail + TAIL_OA0, 8, lane, hl ? 0.0f : 1.0f);
      f32x16 t3 = (f32x16)(0.0f);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float t = t2[r];
        t = D.raytrans_elu ? (t > 0.0f ? t : (expf(t) - 1.0f)) : fmaxf(t, 0.0f);
        step1(t3, tail + TAIL_OA2, r, lane, t);
      }
      step1(t3, tail + TAIL_OA2, 8, lane, hl ? 0.0f : 1.0f);
      sigma = fmaxf(t3[0], 0.0f);  // output row 0 <-> register 0 of the lower half-wave
    }
    if (D.density_maskfill && n_valid < 1.0f) sigma = 0.0f;
    if (hl == 0) {
      rs_lds[s_local * 4 + 3] = sigma;
      if (dbg_sigma && ray_ok && jp < S) dbg_sigma[gs] = sigma;
    }
    __syncthreads();
    // every weight / scratch read of this tile is complete: start the DMA of the next tile's first
    // weight segment now, under the compositing
    {
      seg0_in_flight = tile + tile_step < tile_end;
#ifdef MNERF_FUSED_DEBUG
      if (dflags & 4u) seg0_in_flight = false;
#endif
      if (seg0_in_flight) prefetch_segment<NW>(D.wstream, sch, 0, wbuf0_lds, wave, lane);
    }

    TL_STAMP(12);
    // ============================================================ compositing (K5)
    for (int rt = wave; rt < rays_per_tile; rt += NW) {
      const int rr = tile * rays_per_tile + rt;
      if (rr >= R.n_rays || !out_rgb) continue;  // wave-uniform (no compositing in the per-sample entry point)
      float rlen = 1.0f;
      if (!D.wo_render_interval) {
        const RayGeom gg = make_ray(R, rr);
        rlen = sqrtf(gg.rx * gg.rx + gg.ry * gg.ry + gg.rz * gg.rz);
      }
      float carry = 0.f, ar = 0.f, ag = 0.f, ab = 0.f, ad = 0.f, ao = 0.f;
      for (int j0 = 0; j0 < S; j0 += 64) {
        const int jj = j0 + lane;
        const bool ok = jj < S;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        float dd = 0.f;
        if (ok) {
          c = reinterpret_cast<const float4*>(rs_lds)[rt * Sp + jj];
          dd = sample_depth(R, rr, jj);
          if (!D.wo_render_interval) {
            const float intv = (jj + 1 < S) ? (sample_depth(R, rr, jj + 1) - dd) : 1e10f;
            c.w = c.w * (intv * rlen);
          }
        }
        // exclusive prefix of sigma*delta: scan the lane-shifted values (see composite.hip)
        float incl = __shfl_up(c.w, 1, 64);
        if (lane == 0) incl = 0.0f;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const float t = __shfl_up(incl, off, 64);
          if (lane >= off) incl += t;
        }
        const float excl = carry + incl;
        const float w = ok ? expf(-excl) * (1.0f - expf(-c.w)) : 0.0f;
        ar += w * c.x;
        ag += w * c.y;
        ab += w * c.z;
        ad += w * dd;
        ao += w;
        carry = __shfl(excl + c.w, 63, 64);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        ar += __shfl_xor(ar, off, 64);
        ag += __shfl_xor(ag, off, 64);
        ab += __shfl_xor(ab, off, 64);
        ad += __shfl_xor(ad, off, 64);
        ao += __shfl_xor(ao, off, 64);
      }
      if (lane == 0) {
        const float bg = D.setbg_opaque ? (1.0f - ao) : 0.0f;
        out_rgb[(size_t)rr * 3 + 0] = ar + bg;
        out_rgb[(size_t)rr * 3 + 1] = ag + bg;
        out_rgb[(size_t)rr * 3 + 2] = ab + bg;
        out_depth[rr] = ad;
        out_opacity[rr] = ao;
      }
    }
    TL_STAMP(13);
#ifdef MNERF_TIMELINE
    if (sch.tl && lane == 0 && tl_slot >= 0 && tl_tile < 4) {
      sch.tl[(((size_t)tl_slot * 4 + tl_tile) * NW + wave) * TL_POINTS + 15] = tl_dma_wait;
      sch.tl[(((size_t)tl_slot * 4 + tl_tile) * NW + wave) * TL_POINTS + 16] = tl_bar_wait;
    }
#endif
    // No barrier here: the next tile touches rs_lds only after several segment barriers,
    // and every read of the attention scratch (aliased on the weight buffers that the next
    // tile's first DMA overwrites) completed before the barrier in front of the compositing.
    TL_STAMP(14);
  }
}

// ------------------------------------------------------------------ host side
// one instance: persistent grid (2 workgroups per CU x 256 CUs by default), its LDS attribute set once per device
template <int NW, int SP, int FMT, int CVF>
static void launch_staged_instance(const DecCall& c, const DecSched& sch) {
  const int resident = mnerf_tune().decoder_grid;
  const int rpt = (NW * 32) / SP;
  const int tiles = (c.rays->n_rays + rpt - 1) / rpt;
  const int grid = tiles < resident ? tiles : resident;
  size_t lds = Smem<NW, SP>::TOTAL_FLOATS * sizeof(float);
  static std::atomic<unsigned long long> attr_set{0};
  bool set_attr = mnerf_once_per_device(attr_set);
#ifdef MNERF_FUSED_DEBUG
  // debug build of the one-launch form (tools/exp/race_probe.py): MNERF_FDBG_LDS_KB reserves that much LDS per workgroup instead of
  // the natural footprint (0 = natural), and may change from one launch to the next
  if (const char* e = CVF ? getenv("MNERF_FDBG_LDS_KB") : nullptr) {
    if (atoi(e)) lds = (size_t)atoi(e) * 1024;
  }
  set_attr = true;
#endif
  if (set_attr)
    (void)hipFuncSetAttribute((const void*)decoder_kernel<NW, SP, FMT, CVF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  static const mnerf_scene no_scene = {};
  hipLaunchKernelGGL((decoder_kernel<NW, SP, FMT, CVF>), dim3(grid), dim3(NW * 64), lds, (hipStream_t)c.stream, *c.dec, sch, *c.view0,
                     *c.rays, c.cond, c.rgb, c.depth, c.opacity, c.rgb_s, c.sigma, c.ext_ndc, c.ext_dir,
                     c.fused_scene ? *c.fused_scene : no_scene);
}

// the matrix path by the stream's format; the one-launch form exists for the split-fp16 stream only
template <int NW, int SP, int CVF>
static void launch_staged_format(const DecCall& c, const DecSched& sch) {
  if constexpr (CVF)
    launch_staged_instance<NW, SP, 2, 1>(c, sch);
  else if (c.dec->wstream_format == MNERF_WSTREAM_F16X2)
    launch_staged_instance<NW, SP, 2, 0>(c, sch);
  else if (c.dec->wstream_format == MNERF_WSTREAM_BF16X3)
    launch_staged_instance<NW, SP, 1, 0>(c, sch);
  else
    launch_staged_instance<NW, SP, 0, 0>(c, sch);
}

// Launch the staged form (CVF = 0) or the one-launch form (CVF = 1) for a call that check_decoder_call has passed.
template <int CVF>
static int launch_staged(const DecCall& c, const DecSched& sch, int Sp) {
  const char* who = c.who;
  MNERF_REQUIRE(c.dec->wstream_format != MNERF_WSTREAM_F16X1, MNERF_E_UNSUPPORTED,
                "%s: the one-product fp16 mode (MNERF_WSTREAM_F16X1) exists in the ping-pong decoder only (<= 5 source views, "
                "sample_intvs <= 128, MNERF_DECODER_PP on, not the one-launch form)", who);
  MNERF_REQUIRE(!c.rays->pose_table, MNERF_E_UNSUPPORTED, "%s: a pose table needs the ping-pong decoder (split-fp16 stream, <= 5 source views, "
                "sample_intvs <= 128, MNERF_DECODER_PP on)", who);
  switch (Sp) {
    case 32: launch_staged_format<4, 32, CVF>(c, sch); break;
    case 64: launch_staged_format<4, 64, CVF>(c, sch); break;
    case 128: launch_staged_format<4, 128, CVF>(c, sch); break;
    default:  // 128 < S <= 256 when the ping-pong form does not apply (other stream formats, 6+ views, MNERF_DECODER_PP_MAX_S < 256):
              // one 8-wave workgroup per CU, VALU ray attention
      if constexpr (CVF)
        MNERF_REQUIRE(false, MNERF_E_UNSUPPORTED, "%s: the one-launch form needs sample_intvs <= 128", who);
      else
        launch_staged_format<8, 256, 0>(c, sch);
      break;
  }
  return mnerf_check_launch(who);
}
