// 3x3 stride-1 pad-1 convolution on v_mfma_f32_16x16x32_bf16 with the operands in bf16, ONE body template
// conv_halo_k32_bf16<BN, WAVES_N, TERMS> behind conv_halo_k32_x1_kernel and conv_halo_k32_x2_kernel, the two opt-in precisions: fp32 tensors in HBM, each operand turned into TERMS
// bf16 terms ONCE, fp32 accumulation.
//   TERMS = 1  'bf16x1' (ops.conv2d_bf16x1, ops.infer_precision / train_precision('bf16x1')): x1 = (__bf16)x, round to nearest even
//              (the first term of split3_4 in mfma_split.h), one MFMA per product.  One sixth of the matrix instructions and one
//              third of the LDS operand bytes of conv_halo_k32_kernel (conv_igemm_halo_k32.hip), whose data flow this keeps; an
//              APPROXIMATION (relative operand error 2^-9 each).
//   TERMS = 2  'bf16x2' (ops.conv2d(..., precision='bf16x2')): x = x1 + x2 + (residual <= 2^-16 |x|) (split2 in mfma_split.h:
//              x1 = bf16_rne(x), x2 = bf16_rne(x - x1), the subtraction exact), three MFMAs per product in a fixed order, small
//              terms first:   acc += x1 * w2;  acc += x2 * w1;  acc += x1 * w1     (x2 * w2 and every third-term product are
//              dropped): |x w - (x1 w1 + x1 w2 + x2 w1)| <= (3 * 2^-16 + 3 * 2^-32) |x w|.  Half the matrix instructions of
//              conv_halo_k32_kernel, three times those of TERMS = 1.  With the second terms exactly zero the two extra sweeps
//              add zeros: the result is TERMS = 1's.
// Nothing routes here unless the caller asks.
// Data flow per workgroup (8 rows x 32 pixels x BN output channels; waves = 4 x BN/64, each 64 pixels x 64 channels):
//   weights  [Cout tile][step = chunk32 * 9 + tap][plane][fragment j][lane][16 B]  (ssg_pack_weights_bf16x1, fmt 1128 / 1064: the
//            k32 layout with one plane; ssg_pack_weights_bf16x2, fmt 2128 / 2064: two) -> ring of 3 stages by LDS-DMA in
//            lane-linear 1-KiB pieces; a stage is BN * 128 B, contiguous in the pack, two pieces per wave.  One term: a stage
//            holds TWO steps, piece j of a wave lies in step + j.  Two terms: ONE step, both planes, piece j lies in plane j;
//   pixels   fp32 NHWC -> registers (buffer loads, 8 halo pixels x the chunk's 128 B per instruction; out-of-image lanes read
//            zeros through the descriptor's range check) -> (__bf16) / split2_4 -> TERMS LDS images [plane][k-group][NPIX][16 B],
//            single-buffered: the loads of chunk c+1 are issued in the first interval of chunk c, converted behind its last MFMA
//            (the two planes take the registers the raw values leave), written between two barriers at the chunk boundary.
// Barrier interval -- the one real difference between the two, kept as two separate main loops:
//   TERMS = 1  a step is 16 MFMAs per wave (~256 cycles; the three-term kernel has 96), so one workgroup barrier and one DMA
//              issue cover TWO taps: the nine taps of a chunk run as intervals (0,1) (2,3) (4,5) (6,7) (8) -- 1.8 steps per
//              barrier, the ring stage a runtime counter (5 is no multiple of 3).  The last interval's stage has one step: its
//              second piece per wave is issued with every lane out of range, so every interval issues the same two pieces per
//              wave and the vmcnt immediates stay uniform.
//   TERMS = 2  a step is 48 MFMAs per wave (~770 cycles), so an interval is ONE tap: nine intervals per chunk, ring stage =
//              interval % 3 at compile time.  The three terms run as three sweeps over the 16 accumulators, so a dependent MFMA
//              is 16 issues behind its predecessor.
// LDS: TERMS x 23 KB images + 3 x 16 KB ring = 71 / 94 KB for BN = 128, TERMS x 23 + 24 = 47 / 70 KB for BN = 64.  Registers, not LDS,
// set the occupancy: every instantiation needs ~200 VGPRs (64 accumulators; the fragments of two steps, or two planes of 4 pixel
// and 4 weight fragments = 64; the next chunk's pixels), i.e. two waves per SIMD -- ONE 512-thread workgroup per CU for BN = 128
// (at 128 registers it spills 144), TWO 256-thread workgroups per CU for BN = 64 (94 / 140 KB), whose prologues and tails then
// overlap the other's main loop.
// The summation order is fixed by (chunk, tap, term): it does not depend on the grid.
// Non-finite operands (conv_slow.h, the tail in conv_k32_tail.h): kept, and needed more than in the split kernels -- an fp32 value
// above ~3.39e38 (>= 2^128 - 2^119) rounds to bf16 infinity although the fp32 product is finite.  REQUIRED for two terms: an
// infinite x1 makes x - x1 a NaN, so every tile that reads an infinite or bf16-overflowing operand holds a non-finite accumulator.
// A workgroup with a non-finite accumulator recomputes its tile from the fp32 operands, one accumulator row group at a time so
// that the scratch (NI * 4 values per thread) fits the allocation.
#include "common.h"
#include "lds_dma.h"
#include "conv_k32_bf16_host.h"
#include "mfma_split.h"
#include "conv_k32_tail.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int K32_TH = 8, K32_TW = 32;
constexpr int K32_HW = K32_TW + 2, K32_HR = (K32_TH + 2) * K32_HW;
constexpr int K32_NPIX = (K32_HR + 15) / 16 * 16;
constexpr int K32_KGS = K32_NPIX * 16 + 64;             // bytes between k-groups: + 64 B, the 8-byte writes of a pixel's four k-groups land on distinct banks
constexpr int K32_IMG = (4 * K32_KGS + 1023) / 1024 * 1024;
constexpr int lds_bytes_of(int BN, int TERMS) { return TERMS * K32_IMG + 3 * 2 * BN * 64; }      // TERMS pixel planes, three ring stages of BN * 128 B

template <int BN, int WAVES_N, int TERMS>
__device__ __forceinline__ void conv_halo_k32_bf16(const ConvArgs a) {
  constexpr int WAVES_M = 4, NW = WAVES_M * WAVES_N, NT = NW * 64;
  constexpr int TH = K32_TH, TW = K32_TW, HW = K32_HW, HR = K32_HR, KGS = K32_KGS, IMG = K32_IMG;
  constexpr int BSTG = BN * 64;                          // bytes of one plane of one step's weights (one tap x 32 channels)
  constexpr int STEPB = TERMS * BSTG;                    // bytes of a step in the pack
  constexpr int STG = 2 * BSTG;                          // a ring stage: two steps of one plane, or one step of two
  constexpr int B_PC = STG / 1024 / NW;                  // DMA pieces per wave and interval
  constexpr int WTM = 64, WTN = BN / WAVES_N;
  constexpr int MI = WTM / 16, NI = WTN / 16;
  constexpr int NGRP = (HR + 7) / 8, GPW = (NGRP + NW - 1) / NW, NLD = GPW;
  static_assert(TERMS == 1 || TERMS == 2, "one rounded term, or the two of split2");
  static_assert(STG % (1024 * NW) == 0 && B_PC == 2, "two whole 1-KiB pieces per wave and interval");
  static_assert(WTN == 64 && TH * TW == WAVES_M * WTM, "a wave owns two 32-pixel tile rows x 64 channels");
  static_assert(IMG % 1024 == 0, "the ring behind the image stays 1-KiB aligned");
  static_assert(NI * 4 * NT * 4 <= lds_bytes_of(BN, TERMS), "the slow path's scratch (one accumulator row group per thread) fits the LDS allocation");

  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  unsigned char* const img = lds;                        // plane 1 of the pixels at img + IMG
  unsigned char* const ring = lds + TERMS * IMG;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int l15 = lane & 15, kg = lane >> 4;

  const ConvTile tile = ssg_conv_tile(a);
  const int nyt = a.ntiles_n, nt = tile.nt, n0 = nt * BN, tx = tile.tx, ty = tile.ty, n = tile.n;

  const int nchunks = (a.C1 + a.C2) >> 5;
  const int nsteps = nchunks * 9;
  const unsigned OOB = 0xffffffffu;
  const unsigned npix = (unsigned)a.N * (unsigned)a.H * (unsigned)a.W;
  const auto in1_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in1), 0, (int)(npix * (unsigned)a.ld1 * 4u), 0x00020000);
  const auto in2_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in2), 0, (int)(npix * (unsigned)a.ld2 * 4u), 0x00020000);
  const auto w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)((unsigned)nyt * (unsigned)nsteps * (unsigned)STEPB), 0x00020000);
  const unsigned w_tile = (unsigned)nt * (unsigned)nsteps * (unsigned)STEPB;

  // ---- pixel load items of this thread: group (wave * GPW + k) of 8 halo pixels; lane = (pixel p8 of the group, 16-byte quarter q8 of the chunk)
  const int p8 = lane >> 3, q8 = lane & 7;
  const int hp0 = wave * GPW * 8 + p8;                   // halo pixel of item 0; item k: + 8 k
  const int pix_base = (n * a.H + ty * TH - 1) * a.W + tx * TW - 1;
  auto px_pix_of = [&](int k) -> unsigned {              // recomputed where it is used: the hot loop keeps no table
    const int hp = hp0 + 8 * k;
    const int hy = hp / HW, hx = hp - hy * HW;
    const bool ok = hp < HR && (unsigned)(ty * TH + hy - 1) < (unsigned)a.H && (unsigned)(tx * TW + hx - 1) < (unsigned)a.W;
    return ok ? (unsigned)(pix_base + hy * a.W + hx) : OOB;
  };
  const int px_dst0 = (q8 >> 1) * KGS + hp0 * 16 + (q8 & 1) * 8;      // byte offset of item 0 in the image; item k: + 128 k
  u32x4 raw[NLD];
  auto load_px = [&](int chunk) {
    const int c0 = chunk * 32;
    const bool live = chunk < nchunks;                   // past the last chunk: out-of-range lanes keep vmcnt uniform, nothing is fetched
    const bool first = c0 < a.C1;
    const unsigned ld4 = (unsigned)(first ? a.ld1 : a.ld2) * 4u;
    const unsigned so = (unsigned)(first ? c0 : c0 - a.C1) * 4u;
#pragma unroll
    for (int k = 0; k < GPW; ++k) {
      const unsigned pix = px_pix_of(k);
      const unsigned vo = (live && pix != OOB) ? pix * ld4 + (unsigned)q8 * 16u : OOB;
      if (first) raw[k] = __builtin_amdgcn_raw_buffer_load_b128(in1_rs, vo, so, 0);
      else raw[k] = __builtin_amdgcn_raw_buffer_load_b128(in2_rs, vo, so, 0);
    }
  };
  bf16x4 cv[TERMS][GPW];                                 // [plane]
  auto convert_px = [&]() {
#pragma unroll
    for (int k = 0; k < GPW; ++k) {
      const f32x4 v = __builtin_bit_cast(f32x4, raw[k]);
      if constexpr (TERMS == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) cv[0][k][e] = (__bf16)v[e];          // round to nearest even; NaN stays NaN, |x| >= 2^128 - 2^119 becomes inf
      } else {
        split2_4(v, cv[0][k], cv[1][k]);                 // NaN stays NaN; |x| >= 2^128 - 2^119: first term inf, second NaN
      }
    }
  };
  auto write_px = [&]() {
#pragma unroll
    for (int k = 0; k < GPW; ++k)
      if (hp0 + 8 * k < HR) {
#pragma unroll
        for (int h = 0; h < TERMS; ++h) *(bf16x4*)(img + h * IMG + px_dst0 + 128 * k) = cv[h][k];
      }
  };
  // The BN * 128 bytes of the pack from `step` on -> ring stage `stg`, as two pieces per wave, BSTG apart (BSTG is NW pieces).  One
  // term: that is the two steps `step`, `step + 1` (`single`: only the first).  Two terms: the two planes of `step` (`single` is
  // false).  A piece that is not wanted -- the second of a single-step interval, both past the last step -- is issued with every lane
  // out of range (the range check is on the VECTOR offset): nothing is fetched, vmcnt stays uniform.
  auto issue_b = [&](int step, int stg, bool single) {
    unsigned char* st = ring + stg * STG;
    static_assert(BSTG == NW * 1024, "piece j of a wave lies in step + j, or in plane j");
#pragma unroll
    for (int j = 0; j < B_PC; ++j) {
      const bool ok = step < nsteps && !(single && j == 1);
      const unsigned vo = ok ? (unsigned)lane * 16u : OOB;
      const unsigned piece = TERMS == 1 ? (unsigned)(step + j) * (unsigned)BSTG : (unsigned)step * (unsigned)STEPB + (unsigned)j * (unsigned)BSTG;
      const unsigned so = ok ? w_tile + piece + (unsigned)wave * 1024u : 0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (ssg_lds_void*)(st + (wave + NW * j) * 1024), 16, vo, so, 0, 0);
    }
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int pb[MI];                                            // byte offset of this lane's pixel in the image, tap (0, 0)
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int p = wm * WTM + i * 16 + l15;
    pb[i] = kg * KGS + (((p >> 5) + 1) * HW + (p & 31) + 1) * 16;
  }
  const int wfrag = wn * NI * 1024 + lane * 16;          // this lane's 16 bytes of fragment (wn * NI + j) of a step: + j * 1024

  // ---- prologue: pixels of chunk 0 (the oldest vmcnt entries), two weight intervals in flight
  load_px(0);
  issue_b(0, 0, false);
  issue_b(TERMS == 1 ? 2 : 1, 1, false);                 // the second interval: steps 2 and 3, or step 1
  wait_vmcnt<2 * B_PC>();
  convert_px();
  write_px();

  // ---- main loop.  Two schedules, not one with parameters: see "Barrier interval" above.
  if constexpr (TERMS == 1) {
    int stg = 0;                                         // ring stage of the current interval
    for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma unroll
      for (int iv = 0; iv < 5; ++iv) {                   // interval = two taps (the last: one)
        // the pixel loads issued in interval 0 may still be in flight at the top of intervals 1 and 2; they have landed at 3
        if (iv == 1 || iv == 2) wait_vmcnt<B_PC + NLD>();
        else wait_vmcnt<B_PC>();
        wait_lds_reads();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (iv == 0 && chunk > 0) {
          // every wave has left the last tap of the previous chunk: replace the image
          write_px();
          wait_lds_reads();
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
        }
        const unsigned char* st = ring + stg * STG + wfrag;
        const int stg2 = stg == 0 ? 2 : stg - 1;           // (stg + 2) % 3: the stage every wave left at the barrier above
        // interval iv + 2 of this chunk, or iv - 3 of the next
        const int nstep = iv + 2 < 5 ? chunk * 9 + 2 * (iv + 2) : (chunk + 1) * 9 + 2 * (iv - 3);
        // the fragments of BOTH steps are requested before the first MFMA: read into one register set, the second step's reads would
        // wait behind the first step's MFMAs and stall the wave at every step
        const int NH = iv == 4 ? 1 : 2;
        bf16x8 p[2][MI], w[2][NI];
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          const int tb = (int)((a.tap_bits >> (6 * (2 * iv + h))) & 63ull);  // ssg_tap_dy / ssg_tap_dx (common.h) written out
          const int toff = (((tb & 7) - 2) * HW + ((tb >> 3) - 2)) * 16;
#pragma unroll
          for (int i = 0; i < MI; ++i) p[h][i] = *(const bf16x8*)(img + pb[i] + toff);
#pragma unroll
          for (int j = 0; j < NI; ++j) w[h][j] = *(const bf16x8*)(st + h * BSTG + j * 1024);
        }
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          // priority by progress through the interval, as in conv_halo_k32_kernel: the two waves of a SIMD stay together
          if (h == 0) __builtin_amdgcn_s_setprio(2);
          else __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int i = 0; i < MI; ++i) {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[h][j], p[h][i], acc[i][j], 0, 0, 0);
              if (h == 0 && j == NI / 2 - 1 && i == MI - 1) {
                // the DMA pieces (and the next chunk's pixel loads) go out among the MFMAs, not into the burst of fragment reads behind the barrier
                __builtin_amdgcn_sched_barrier(0);
                issue_b(nstep, stg2, iv == 2);
                if (iv == 0) load_px(chunk + 1);
                __builtin_amdgcn_sched_barrier(0);
              }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if (iv == 4) {                                   // the loads of interval 0 landed before interval 3's barrier
          __builtin_amdgcn_sched_barrier(0);
          convert_px();
        }
        stg = stg == 2 ? 0 : stg + 1;
      }
    }
  } else {
    for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma unroll
      for (int iv = 0; iv < 9; ++iv) {                   // interval = tap; nine intervals keep the ring stage at iv % 3
        // the pixel loads issued in interval 0 may still be in flight at the top of intervals 1 and 2; they have landed at 3
        if (iv == 1 || iv == 2) wait_vmcnt<B_PC + NLD>();
        else wait_vmcnt<B_PC>();
        wait_lds_reads();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (iv == 0 && chunk > 0) {
          // every wave has left the last tap of the previous chunk: replace the images
          write_px();
          wait_lds_reads();
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
        }
        const unsigned char* st = ring + (iv % 3) * STG + wfrag;
        const int tb = (int)((a.tap_bits >> (6 * iv)) & 63ull);            // ssg_tap_dy / ssg_tap_dx (common.h) written out
        const int toff = (((tb & 7) - 2) * HW + ((tb >> 3) - 2)) * 16;
        bf16x8 p[2][MI], w[2][NI];                       // [plane]
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int i = 0; i < MI; ++i) p[h][i] = *(const bf16x8*)(img + h * IMG + pb[i] + toff);
#pragma unroll
          for (int j = 0; j < NI; ++j) w[h][j] = *(const bf16x8*)(st + h * BSTG + j * 1024);
        }
        // the three kept products, small terms first: x1 w2, x2 w1, x1 w1 -- one sweep over the accumulators per term
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          // priority by progress through the interval, as in conv_halo_k32_kernel: the two waves of a SIMD stay together
          if (t == 0) __builtin_amdgcn_s_setprio(2);
          else __builtin_amdgcn_s_setprio(1);
          const int hw = t == 0 ? 1 : 0, hp = t == 1 ? 1 : 0;
#pragma unroll
          for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int i = 0; i < MI; ++i) {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[hw][j], p[hp][i], acc[i][j], 0, 0, 0);
              if (t == 0 && j == NI / 2 - 1 && i == MI - 1) {
                // the DMA pieces (and the next chunk's pixel loads) go out among the MFMAs, not into the burst of fragment reads behind the barrier
                __builtin_amdgcn_sched_barrier(0);
                issue_b(chunk * 9 + iv + 2, (iv + 2) % 3, false);          // the stage every wave left at the barrier above
                if (iv == 0) load_px(chunk + 1);
                __builtin_amdgcn_sched_barrier(0);
              }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if (iv == 8) {                                   // the loads of interval 0 landed before interval 3's barrier
          __builtin_amdgcn_sched_barrier(0);
          convert_px();
        }
      }
    }
  }
  wait_vmcnt<0>();
  wait_lds_reads();

  // ---- the tail (conv_k32_tail.h): non-finite recompute over the nine taps, then bias / residual / activation / store
  ssg_k32_recompute_nonfinite<9, TH, WTM, WTN, NT>(acc, lds, tid, n, ty, tx, n0, wm, wn, kg, l15);
  ssg_k32_epilogue<TH, WTM, WTN>(a, acc, n, ty, tx, n0, wm, wn, kg, l15);
}

// The two kernels keep the names their profiling labels and traces have had: one line each over the shared body.
template <int BN, int WAVES_N>
__global__ __launch_bounds__(4 * WAVES_N * 64, 2) void conv_halo_k32_x1_kernel(const ConvArgs a) { conv_halo_k32_bf16<BN, WAVES_N, 1>(a); }
template <int BN, int WAVES_N>
__global__ __launch_bounds__(4 * WAVES_N * 64, 2) void conv_halo_k32_x2_kernel(const ConvArgs a) { conv_halo_k32_bf16<BN, WAVES_N, 2>(a); }

// fp32 packed [R][Kp] (kmode 0 with `ntaps` taps: k = (chunk16 * ntaps + tap) * 16 + c) -> [R / BN][chunk32 * ntaps + tap][TERMS planes]
// [BN / 16 fragments][64 lanes][16 B]: lane l of fragment j holds output channel j*16 + (l & 15), channels chunk32*32 + (l >> 4)*8 .. +7;
// plane 0 = the value rounded to nearest even, plane 1 (two terms) = the rounded residual (split2).  One thread per (row, step,
// k-group).  Nine taps for the unit-stride and stride-2 forward convs, 1 / 2 / 4 for the parity classes of conv_s2_k32_x1.hip.
template <int TERMS>
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ w, int R, int Kp, int ntaps, int BN, unsigned char* __restrict__ out) {
  const int nsteps = Kp >> 5;
  const long long total = (long long)R * nsteps * 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int g = (int)(i & 3);
    long long t = i >> 2;
    const int s = (int)(t % nsteps); t /= nsteps;
    const int row = (int)t;
    const int tile = row / BN, rl = row - tile * BN;
    const int chunk32 = s / ntaps, tap = s - chunk32 * ntaps;
    const int chunk16 = chunk32 * 2 + (g >> 1);
    const float* src = w + (size_t)row * Kp + (size_t)(chunk16 * ntaps + tap) * 16 + (g & 1) * 8;
    const f32x4 u = *(const f32x4*)src, v = *(const f32x4*)(src + 4);
    const int j = rl >> 4, l = (rl & 15) + 16 * g;
    unsigned char* dst = out + ((size_t)tile * nsteps + s) * BN * (64 * TERMS) + (size_t)j * 1024 + (size_t)l * 16;
    if constexpr (TERMS == 1) {
      bf16x8 p;
#pragma unroll
      for (int e = 0; e < 4; ++e) { p[e] = (__bf16)u[e]; p[4 + e] = (__bf16)v[e]; }
      *(bf16x8*)dst = p;
    } else {
      bf16x8 p1, p2;
      split2(u, v, p1, p2);
      *(bf16x8*)dst = p1;
      *(bf16x8*)(dst + (size_t)BN * 64) = p2;
    }
  }
}

template <int BN, int WAVES_N, int TERMS>
int launch(const ConvArgs& a0, hipStream_t st) {
  ConvArgs a = a0;
  const dim3 grid = ssg_conv_tile_grid(a, K32_TW, K32_TH, BN);
  constexpr int lds_bytes = lds_bytes_of(BN, TERMS);
  static_assert(lds_bytes <= 160 * 1024 && (BN != 64 || 2 * lds_bytes <= 160 * 1024), "LDS: two 256-thread workgroups per CU for BN = 64, one 512-thread workgroup for BN = 128");
  if constexpr (TERMS == 1) {
    SSG_DYN_LDS_ONCE((conv_halo_k32_x1_kernel<BN, WAVES_N>), lds_bytes, "conv bf16x1");
    hipLaunchKernelGGL((conv_halo_k32_x1_kernel<BN, WAVES_N>), grid, dim3(4 * WAVES_N * 64), lds_bytes, st, a);
  } else {
    SSG_DYN_LDS_ONCE((conv_halo_k32_x2_kernel<BN, WAVES_N>), lds_bytes, "conv bf16x2");
    hipLaunchKernelGGL((conv_halo_k32_x2_kernel<BN, WAVES_N>), grid, dim3(4 * WAVES_N * 64), lds_bytes, st, a);
  }
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

// ---- host side: the descriptor checks and the launch sequence are conv_k32_bf16_host.h's; here the choice of the kernel, and the
// one pack launcher of the family
constexpr const char* family(int terms) { return terms == 1 ? "bf16x1" : "bf16x2"; }

// 70 / 71 for one term, 90 / 91 for two: BN = 128 / 64
int kernel_id(const ssg_conv_desc* d, int terms) {
  const int fmt = ssg_k32_bf16_conv_fmt(d, K32_UNIT, family(terms), terms);
  return fmt ? (terms == 1 ? 70 : 90) + (fmt % 1000 == 128 ? 0 : 1) : SSG_EINVAL;
}

template <int TERMS>
int run(const ssg_conv_desc* d, const void* pack, void* stream) {
  return ssg_k32_bf16_conv_run(d, pack, K32_UNIT, family(TERMS), TERMS, stream, [](const ConvArgs& a, hipStream_t st) {
    return ssg_k32_bf16_bn(a.Cout) == 128 ? launch<128, 2, TERMS>(a, st) : launch<64, 1, TERMS>(a, st);
  });
}

// Bytes of the pack of [R][Kp] over `ntaps` taps in format BN = 1000 * terms + column tile, or 0 where that is no pack
int64_t pack_bytes(int R, int Kp, int ntaps, int BN, int terms) {
  const int bn = BN - 1000 * terms;
  if (bn != 64 && bn != 128) return 0;
  if (ntaps <= 0 || ntaps > 9 || R <= 0 || R % bn || Kp <= 0 || Kp % (32 * ntaps)) return 0;
  return (int64_t)(R / bn) * (Kp / 32) * bn * 64 * terms;
}

// `who`: the entry point's name in the messages
template <int TERMS>
int pack(const char* who, const float* w_packed, int R, int Kp, int ntaps, int BN, void* out, void* stream) {
  SSG_REQUIRE(w_packed && out && pack_bytes(R, Kp, ntaps, BN, TERMS) > 0, SSG_EINVAL, "pack %s: bad args (R=%d Kp=%d ntaps=%d BN=%d)", who, R, Kp, ntaps, BN);
  SSG_REQUIRE(ssg_aligned16(w_packed) && ssg_aligned16(out), SSG_EALIGN, "pack %s: 16-B alignment", who);
  const long long total = (long long)R * (Kp >> 5) * 4;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(pack_bf16_kernel<TERMS>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w_packed, R, Kp, ntaps, BN - 1000 * TERMS, (unsigned char*)out);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

}  // namespace

// _ok: the pack format code (BN of ssg_pack_weights_bf16x1 / _bf16x2) the launch for `d` reads, or 0 where the launch refuses `d`.
extern "C" int ssg_conv2d_bf16x1_ok(const ssg_conv_desc* d) { return ssg_k32_bf16_conv_fmt(d, K32_UNIT, "bf16x1", 1); }
extern "C" int ssg_conv2d_bf16x1_kernel_id(const ssg_conv_desc* d) { return kernel_id(d, 1); }
extern "C" int ssg_conv2d_bf16x1_f32(const ssg_conv_desc* d, const void* w_bf16x1, void* stream) { return run<1>(d, w_bf16x1, stream); }
extern "C" int ssg_conv2d_bf16x2_ok(const ssg_conv_desc* d) { return ssg_k32_bf16_conv_fmt(d, K32_UNIT, "bf16x2", 2); }
extern "C" int ssg_conv2d_bf16x2_kernel_id(const ssg_conv_desc* d) { return kernel_id(d, 2); }
extern "C" int ssg_conv2d_bf16x2_f32(const ssg_conv_desc* d, const void* w_bf16x2, void* stream) { return run<2>(d, w_bf16x2, stream); }

// The packs: nine taps for the unit-stride and the stride-2 forward launches, the caller's tap count (1 .. 9; one term) for the
// parity classes of conv_s2_k32_x1.hip
extern "C" int64_t ssg_pack_weights_bf16x1_bytes(int R, int Kp, int BN) { return pack_bytes(R, Kp, 9, BN, 1); }
extern "C" int ssg_pack_weights_bf16x1(const float* w_packed, int R, int Kp, int BN, void* out, void* stream) { return pack<1>("bf16x1", w_packed, R, Kp, 9, BN, out, stream); }
extern "C" int64_t ssg_pack_weights_bf16x2_bytes(int R, int Kp, int BN) { return pack_bytes(R, Kp, 9, BN, 2); }
extern "C" int ssg_pack_weights_bf16x2(const float* w_packed, int R, int Kp, int BN, void* out, void* stream) { return pack<2>("bf16x2", w_packed, R, Kp, 9, BN, out, stream); }
extern "C" int64_t ssg_pack_weights_bf16x1_taps_bytes(int R, int Kp, int ntaps, int BN) { return pack_bytes(R, Kp, ntaps, BN, 1); }
extern "C" int ssg_pack_weights_bf16x1_taps(const float* w_packed, int R, int Kp, int ntaps, int BN, void* out, void* stream) {
  return pack<1>("bf16x1 taps", w_packed, R, Kp, ntaps, BN, out, stream);
}
