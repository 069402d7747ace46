// 3x3 stride-1 pad-1 convolution, TWO-TERM form on v_mfma_f32_16x16x32_bf16 (opt-in precision 'bf16x2'): fp32 tensors in HBM,
// each operand split ONCE into two bf16 terms x = x1 + x2 + (residual <= 2^-16 |x|) (split2 in mfma_split.h: x1 = bf16_rne(x),
// x2 = bf16_rne(x - x1), the subtraction exact), three MFMAs per product in a fixed order, small terms first:
//   acc += x1 * w2;  acc += x2 * w1;  acc += x1 * w1        (x2 * w2 and every third-term product are dropped)
// |x w - (x1 w1 + x1 w2 + x2 w1)| <= (3 * 2^-16 + 3 * 2^-32) |x w|; fp32 accumulation.  Half the matrix instructions of
// conv_halo_k32_kernel (conv_igemm_halo_k32.hip), three times those of conv_halo_k32_x2_kernel, whose body this is with both LDS
// images doubled.  Nothing routes here unless the caller asks (ops.conv2d(..., precision='bf16x2')).
// Data flow per workgroup (8 rows x 32 pixels x BN output channels; waves = 4 x BN/64, each 64 pixels x 64 channels):
//   weights  [Cout tile][step = chunk32 * 9 + tap][plane][fragment j][lane][16 B]  (ssg_pack_weights_bf16x2, fmt 2128 / 2064)
//            -> ring of 3 stages by LDS-DMA in lane-linear 1-KiB pieces; a stage holds ONE step, both planes (BN * 128 B,
//            contiguous in the pack), two pieces per wave: piece j of a wave lies in plane j;
//   pixels   fp32 NHWC -> registers (buffer loads, 8 halo pixels x the chunk's 128 B per instruction; out-of-image lanes read
//            zeros through the descriptor's range check) -> split2_4 -> two LDS images [plane][k-group][NPIX][16 B],
//            single-buffered: the loads of chunk c+1 are issued in the first interval of chunk c, split behind its last MFMA
//            (the two planes take the registers the raw values leave), written between two barriers at the chunk boundary.
// Barrier interval: a step is 48 MFMAs per wave (~770 cycles; the one-term kernel has 16 and so covers two taps per barrier), so
// an interval is ONE tap: nine intervals per chunk, ring stage = interval % 3 at compile time.  The three terms run as three
// sweeps over the 16 accumulators, so a dependent MFMA is 16 issues behind its predecessor.
// LDS: 2 x 23 KB images + 3 x 16 KB ring = 94 KB for BN = 128 (one 512-thread workgroup per CU), 46 + 24 = 70 KB for BN = 64 (two
// 256-thread workgroups per CU, 140 KB).  Registers: 64 accumulators, 64 of fragments (two planes of 4 pixel and 4 weight
// fragments), the next chunk's pixels; two waves per SIMD as in the one-term kernel.
// The summation order is fixed by (chunk, tap, term): it does not depend on the grid.
// Non-finite operands (conv_slow.h): REQUIRED here -- an infinite x1 makes x - x1 a NaN, so every tile that reads an infinite or
// bf16-overflowing (>= 2^128 - 2^119) operand holds a non-finite accumulator and is recomputed from the fp32 operands, one
// accumulator row group at a time so that the scratch (NI * 4 values per thread) fits the allocation.
#include "common.h"
#include "lds_dma.h"
#include "conv_args.h"
#include "mfma_split.h"
#include "conv_slow.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int X2_TH = 8, X2_TW = 32;
constexpr int X2_HW = X2_TW + 2, X2_HR = (X2_TH + 2) * X2_HW;
constexpr int X2_NPIX = (X2_HR + 15) / 16 * 16;
constexpr int X2_KGS = X2_NPIX * 16 + 64;               // bytes between k-groups: + 64 B, the 8-byte writes of a pixel's four k-groups land on distinct banks
constexpr int X2_IMG = (4 * X2_KGS + 1023) / 1024 * 1024;
constexpr int x2_lds_bytes(int BN) { return 2 * X2_IMG + 3 * 2 * BN * 64; }      // two pixel planes, three stages of one step x two planes

template <int BN, int WAVES_N>
__global__ __launch_bounds__(4 * WAVES_N * 64, 2) void conv_halo_k32_x2_kernel(const ConvArgs a) {
  constexpr int WAVES_M = 4, NW = WAVES_M * WAVES_N, NT = NW * 64;
  constexpr int TH = X2_TH, TW = X2_TW, HW = X2_HW, HR = X2_HR, KGS = X2_KGS, IMG = X2_IMG;
  constexpr int BSTG = BN * 64;                          // bytes of one plane of one step's weights (one tap x 32 channels)
  constexpr int STG = 2 * BSTG;                          // a ring stage: one step, two planes
  constexpr int B_PC = STG / 1024 / NW;                  // DMA pieces per wave and interval
  constexpr int WTM = 64, WTN = BN / WAVES_N;
  constexpr int MI = WTM / 16, NI = WTN / 16;
  constexpr int NGRP = (HR + 7) / 8, GPW = (NGRP + NW - 1) / NW, NLD = GPW;
  static_assert(STG % (1024 * NW) == 0 && B_PC == 2, "two whole 1-KiB pieces per wave and interval");
  static_assert(WTN == 64 && TH * TW == WAVES_M * WTM, "a wave owns two 32-pixel tile rows x 64 channels");
  static_assert(IMG % 1024 == 0, "the ring behind the image stays 1-KiB aligned");
  static_assert(NI * 4 * NT * 4 <= x2_lds_bytes(BN), "the slow path's scratch (one accumulator row group per thread) fits the LDS allocation");

  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  unsigned char* const img = lds;
  unsigned char* const ring = lds + 2 * IMG;             // plane 1 of the pixels at img + IMG

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
  const auto w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)((unsigned)nyt * (unsigned)nsteps * (unsigned)STG), 0x00020000);
  const unsigned w_tile = (unsigned)nt * (unsigned)nsteps * (unsigned)STG;

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
  bf16x4 cv1[GPW], cv2[GPW];
  auto convert_px = [&]() {
#pragma unroll
    for (int k = 0; k < GPW; ++k) split2_4(__builtin_bit_cast(f32x4, raw[k]), cv1[k], cv2[k]);
  };
  auto write_px = [&]() {
#pragma unroll
    for (int k = 0; k < GPW; ++k)
      if (hp0 + 8 * k < HR) {
        *(bf16x4*)(img + px_dst0 + 128 * k) = cv1[k];
        *(bf16x4*)(img + IMG + px_dst0 + 128 * k) = cv2[k];
      }
  };
  // step `step` (both planes) -> ring stage `stg`.  Piece j of a wave lies in plane j (a plane is NW pieces).  Past the last step
  // the pieces are issued with every lane out of range (the range check is on the VECTOR offset): nothing is fetched, vmcnt
  // stays uniform.
  auto issue_b = [&](int step, int stg) {
    unsigned char* st = ring + stg * STG;
    static_assert(BSTG == NW * 1024, "piece j of a wave lies in plane j");
    const bool ok = step < nsteps;
#pragma unroll
    for (int j = 0; j < B_PC; ++j) {
      const unsigned vo = ok ? (unsigned)lane * 16u : OOB;
      const unsigned so = ok ? w_tile + (unsigned)step * (unsigned)STG + (unsigned)j * (unsigned)BSTG + (unsigned)wave * 1024u : 0u;
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
  issue_b(0, 0);
  issue_b(1, 1);
  wait_vmcnt<2 * B_PC>();
  convert_px();
  write_px();

  for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma unroll
    for (int iv = 0; iv < 9; ++iv) {                     // interval = tap; nine intervals keep the ring stage at iv % 3
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
      const int tb = (int)((a.tap_bits >> (6 * iv)) & 63ull);              // ssg_tap_dy / ssg_tap_dx (common.h) written out
      const int toff = (((tb & 7) - 2) * HW + ((tb >> 3) - 2)) * 16;
      bf16x8 p[2][MI], w[2][NI];                         // [plane]
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
              issue_b(chunk * 9 + iv + 2, (iv + 2) % 3);             // the stage every wave left at the barrier above
              if (iv == 0) load_px(chunk + 1);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
      }
      __builtin_amdgcn_s_setprio(0);
      if (iv == 8) {                                     // the loads of interval 0 landed before interval 3's barrier
        __builtin_amdgcn_sched_barrier(0);
        convert_px();
      }
    }
  }
  wait_vmcnt<0>();
  wait_lds_reads();

  // ---- non-finite operands (conv_slow.h): a workgroup that holds a non-finite accumulator recomputes its tile with fp32 FMAs
  {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) bad |= ssg_nonfinite(acc[i][j][r]);
    if (ssg_any_nonfinite(bad)) {
      float* scr = (float*)lds + tid;                    // value e of this thread at scr[e * NT]; only this thread reads it back
      const ConvArgs& as = *ssg_reload_args<ConvArgs>();
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int p = wm * WTM + i * 16 + l15;
#pragma unroll 1
        for (int e = 0; e < NI * 4; ++e) {
          const int co = n0 + wn * WTN + (e >> 2) * 16 + kg * 4 + (e & 3);
          scr[e * NT] = ssg_conv_slow_value<false>(as, n, ty * TH + (p >> 5), tx * TW + (p & 31), co, 0, 9);
        }
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][r] = scr[(j * 4 + r) * NT];
      }
    }
  }

  // ---- epilogue.  acc[i][j][r]: pixel p = wm*64 + i*16 + l15, output channel n0 + wn*64 + j*16 + kg*4 + r.
  size_t opix[MI]; bool pok[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int p = wm * WTM + i * 16 + l15;
    const int gy = ty * TH + (p >> 5), gx = tx * TW + (p & 31);
    pok[i] = gy < a.GH && gx < a.GW;
    opix[i] = (size_t)(n * a.OH + gy) * a.OW + gx;
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int co = n0 + wn * WTN + j * 16 + kg * 4;      // Cout % BN == 0: every column is real
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) bv = *(const f32x4*)(a.bias + co);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if (!pok[i]) continue;
      f32x4 v = acc[i][j] + bv;
      if (a.res) v += *(const f32x4*)(a.res + opix[i] * a.ldr + co);
      if (a.act == SSG_ACT_RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] < 0.f ? 0.f : v[r];
      } else if (a.act == SSG_ACT_LRELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : v[r] * a.slope;
      }
      *(f32x4*)(a.out + opix[i] * a.ldo + co) = v;
    }
  }
}

// fp32 packed [R][Kp] (kmode 0 with 9 taps: k = (chunk16 * 9 + tap) * 16 + c) -> [R / BN][chunk32 * 9 + tap][2 planes][BN / 16 fragments]
// [64 lanes][16 B]: lane l of fragment j holds output channel j*16 + (l & 15), channels chunk32*32 + (l >> 4)*8 .. +7; plane 0 = the
// value rounded to nearest even, plane 1 = the rounded residual (split2).  One thread per (row, step, k-group).
__global__ __launch_bounds__(256) void pack_bf16x2_kernel(const float* __restrict__ w, int R, int Kp, int BN, unsigned char* __restrict__ out) {
  const int nsteps = Kp >> 5;
  const long long total = (long long)R * nsteps * 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int g = (int)(i & 3);
    long long t = i >> 2;
    const int s = (int)(t % nsteps); t /= nsteps;
    const int row = (int)t;
    const int tile = row / BN, rl = row - tile * BN;
    const int chunk32 = s / 9, tap = s - chunk32 * 9;
    const int chunk16 = chunk32 * 2 + (g >> 1);
    const float* src = w + (size_t)row * Kp + (size_t)(chunk16 * 9 + tap) * 16 + (g & 1) * 8;
    bf16x8 p1, p2;
    split2(*(const f32x4*)src, *(const f32x4*)(src + 4), p1, p2);
    const int j = rl >> 4, l = (rl & 15) + 16 * g;
    unsigned char* dst = out + ((size_t)tile * nsteps + s) * BN * 128 + (size_t)j * 1024 + (size_t)l * 16;
    *(bf16x8*)dst = p1;
    *(bf16x8*)(dst + (size_t)BN * 64) = p2;
  }
}

template <int BN, int WAVES_N>
int launch(const ConvArgs& a0, hipStream_t st) {
  ConvArgs a = a0;
  const dim3 grid = ssg_conv_tile_grid(a, X2_TW, X2_TH, BN);
  constexpr int lds_bytes = x2_lds_bytes(BN);
  static_assert(lds_bytes <= 160 * 1024 && (BN != 64 || 2 * lds_bytes <= 160 * 1024), "LDS: two 256-thread workgroups per CU for BN = 64, one 512-thread workgroup for BN = 128");
  SSG_DYN_LDS_ONCE((conv_halo_k32_x2_kernel<BN, WAVES_N>), lds_bytes, "conv bf16x2");
  hipLaunchKernelGGL((conv_halo_k32_x2_kernel<BN, WAVES_N>), grid, dim3(4 * WAVES_N * 64), lds_bytes, st, a);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

// The descriptor as the kernel's argument block; false (with the reason in ssg_last_error when `why`) where the kernel does not take it.
bool x2_args(const ssg_conv_desc* d, ConvArgs& a, bool why) {
#define X2_NEED(cond, ...) do { if (!(cond)) { if (why) ssg_set_error(__VA_ARGS__); return false; } } while (0)
  X2_NEED(d != nullptr, "conv bf16x2: null desc");
  X2_NEED(d->in1 && d->w && d->out, "conv bf16x2: null pointer");
  X2_NEED(!d->bnpart && !d->ws && !d->parity_merge && !d->in_scale && !d->in_shift && !d->bwd_x, "conv bf16x2: bnpart / ws / parity_merge / in_scale / bwd_x are not taken");
  X2_NEED(d->ntaps == 9 && d->kmode == 0 && d->in_sy == 1 && d->in_sx == 1 && d->out_sy == 1 && d->out_sx == 1 && d->out_oy == 0 && d->out_ox == 0,
          "conv bf16x2: the 9 taps of a unit-stride forward conv in kmode 0 only");
  X2_NEED(d->C1 > 0 && d->C1 % 32 == 0 && d->C2 >= 0 && d->C2 % 32 == 0 && (d->C2 == 0 || d->in2), "conv bf16x2: C1=%d C2=%d must be multiples of 32", d->C1, d->C2);
  X2_NEED(d->Cout > 0 && d->Cout % 64 == 0, "conv bf16x2: Cout=%d must be a multiple of 64", d->Cout);
  X2_NEED(d->Kp == (d->C1 + d->C2) * 9, "conv bf16x2: Kp=%d != Cin*9", d->Kp);
  X2_NEED(d->N > 0 && d->H > 0 && d->W > 0 && d->GH > 0 && d->GW >= 17, "conv bf16x2: empty grid or GW=%d < 17", d->GW);
  X2_NEED(d->GH <= d->OH && d->GW <= d->OW, "conv bf16x2: pixel grid exceeds the output image");
  X2_NEED(d->ld1 >= d->C1 && d->ld1 % 4 == 0 && (d->C2 == 0 || (d->ld2 >= d->C2 && d->ld2 % 4 == 0)) && d->ldo >= d->Cout && d->ldo % 4 == 0 &&
          (!d->res || (d->ldr >= d->Cout && d->ldr % 4 == 0)), "conv bf16x2: pixel strides");
  X2_NEED(ssg_aligned16(d->in1) && (d->C2 == 0 || ssg_aligned16(d->in2)) && ssg_aligned16(d->w) && ssg_aligned16(d->out) && ssg_aligned16(d->res) && ssg_aligned16(d->bias),
          "conv bf16x2: 16-B alignment");
  X2_NEED(d->act == SSG_ACT_NONE || d->act == SSG_ACT_RELU || d->act == SSG_ACT_LRELU, "conv bf16x2: act=%d", d->act);
  for (int t = 0; t < 9; ++t) X2_NEED(d->dy[t] >= -1 && d->dy[t] <= 1 && d->dx[t] >= -1 && d->dx[t] <= 1, "conv bf16x2: tap offset outside the 3x3 window");
  const unsigned long long bytes = (unsigned long long)d->N * d->H * d->W * (unsigned long long)(d->ld1 > d->ld2 ? d->ld1 : d->ld2) * 4ull;
  X2_NEED(bytes <= 0xfffffff0ull, "conv bf16x2: input beyond the 32-bit byte offsets of the buffer descriptors");
  X2_NEED((unsigned long long)d->Cout * d->Kp * 4ull <= 0x7ffffff0ull, "conv bf16x2: weight pack beyond the 32-bit byte offsets");
  a = ConvArgs{};
  a.in1 = d->in1; a.in2 = d->C2 ? d->in2 : d->in1; a.bias = d->bias; a.res = d->res; a.out = d->out;
  a.C1 = d->C1; a.C2 = d->C2; a.ld1 = d->ld1; a.ld2 = d->C2 ? d->ld2 : d->ld1;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Kp = d->Kp; a.kmode = 0;
  a.ldr = d->ldr; a.Cout = d->Cout; a.ldo = d->ldo;
  a.GH = d->GH; a.GW = d->GW; a.OH = d->OH; a.OW = d->OW;
  a.in_sy = a.in_sx = a.out_sy = a.out_sx = 1;
  a.ntaps = 9;
  a.tap_bits = ssg_pack_taps(d->dy, d->dx, 9);
  a.act = d->act; a.slope = d->slope;
  a.nsteps = d->Kp / 16; a.ksplit = 1;
  a.w32 = d->w;                                          // the slow path's fp32 weights
  X2_NEED(ssg_conv_halo_ok(a), "conv bf16x2: the taps are not the nine of a 3x3 window");
#undef X2_NEED
  return true;
}

int x2_fmt(const ConvArgs& a) { return a.Cout % 128 == 0 ? 2128 : 2064; }

}  // namespace

// Pack format code (BN of ssg_pack_weights_bf16x2) the launch for `d` reads, or 0 where ssg_conv2d_bf16x2_f32 refuses `d`.
extern "C" int ssg_conv2d_bf16x2_ok(const ssg_conv_desc* d) {
  ConvArgs a;
  return x2_args(d, a, false) ? x2_fmt(a) : 0;
}

extern "C" int ssg_conv2d_bf16x2_kernel_id(const ssg_conv_desc* d) {
  const int fmt = ssg_conv2d_bf16x2_ok(d);
  return fmt == 2128 ? 90 : fmt == 2064 ? 91 : SSG_EINVAL;
}

extern "C" int ssg_conv2d_bf16x2_f32(const ssg_conv_desc* d, const void* w_bf16x2, void* stream) {
  ConvArgs a;
  if (!x2_args(d, a, true)) return SSG_EINVAL;
  SSG_REQUIRE(w_bf16x2 != nullptr, SSG_EINVAL, "conv bf16x2: null weight pack");
  SSG_REQUIRE(ssg_aligned16(w_bf16x2), SSG_EALIGN, "conv bf16x2: weight pack alignment");
  a.w = (const float*)w_bf16x2;
  if (x2_fmt(a) == 2128) return launch<128, 2>(a, (hipStream_t)stream);
  return launch<64, 1>(a, (hipStream_t)stream);
}

extern "C" int64_t ssg_pack_weights_bf16x2_bytes(int R, int Kp, int BN) {
  if (BN != 2064 && BN != 2128) return 0;
  const int bn = BN - 2000;
  if (R <= 0 || R % bn || Kp <= 0 || Kp % (32 * 9)) return 0;
  return (int64_t)(R / bn) * (Kp / 32) * bn * 128;
}

extern "C" int ssg_pack_weights_bf16x2(const float* w_packed, int R, int Kp, int BN, void* out, void* stream) {
  SSG_REQUIRE(w_packed && out && ssg_pack_weights_bf16x2_bytes(R, Kp, BN) > 0, SSG_EINVAL, "pack bf16x2: bad args (R=%d Kp=%d BN=%d)", R, Kp, BN);
  SSG_REQUIRE(ssg_aligned16(w_packed) && ssg_aligned16(out), SSG_EALIGN, "pack bf16x2: 16-B alignment");
  const long long total = (long long)R * (Kp >> 5) * 4;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(pack_bf16x2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w_packed, R, Kp, BN - 2000, (unsigned char*)out);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}
