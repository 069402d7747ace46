// One-term bf16 (bf16x1) kernels for the 3x3 STRIDE-2 pad-1 convolution and for its input gradient, the one-term contract of
// conv_halo_k32_bf16.hip: fp32 NHWC tensors in HBM, both operands rounded ONCE with (__bf16)v (round to nearest even) on the way
// into LDS, one v_mfma_f32_16x16x32_bf16 per product, fp32 accumulation, bias / activation / output in fp32, the non-finite guard
// of conv_slow.h kept; the tail (recompute and epilogue) is conv_k32_tail.h's, shared with that file.  No bnpart, ws, in_scale,
// bwd_x, no residual.  An APPROXIMATION, so nothing routes here unless the caller asks (ops.conv2d(..., precision='bf16x1') from
// the single-conv node).
// One kernel template, conv_s2_k32_x1_kernel<BN, WAVES_N, NTAPS, S>, the data flow of conv_halo_k32_x1_kernel
// (weight ring of 3 two-step stages fed by LDS-DMA from the one-plane 1128 / 1064 pack; pixel image [k-group][pixel][16 B] per
// 32-channel chunk, single-buffered, the next chunk's pixels prefetched into registers), with the tap count a template parameter:
//   (a) forward, S = 2, NTAPS = 9: tiles of TH x 32 = 4 x 32 outputs; the image is the (2 TH + 1) x 65 = 9 x 65-pixel window.
//       A tap (ky, kx) of output (py, px) is window pixel (2 py + ky, 2 px + kx): stored row-major that is a 32-byte lane stride,
//       and the 16 lanes of a ds_read_b128 quarter-wave would span 512 B = twice the 64 banks x 4 B (a two-way conflict on every
//       fragment read).  The window's even and odd COLUMNS are therefore stored as two planes per row ([33 even][32 odd]): column
//       2 px + kx is even-plane px, odd-plane px, even-plane px + 1 for kx = 0, 1, 2 -- every tap a unit-stride read again, at the
//       price of one extra shift / and per pixel WRITE (once per chunk, not once per tap).  Bank arithmetic, not a measurement.
//       TH = 4, not 8: at TH = 8 the window is 1105 pixels = 71 KB per chunk (one workgroup per CU beside the ring) and, with the
//       stride-1 kernel's register prefetch of the next chunk, 35 x 4 VGPRs per thread of a 256-thread workgroup; at TH = 4 it is
//       585 pixels = 38 KB, 19 x 4 VGPRs, LDS 38 + 24 = 62 KB for BN = 64 (TWO 256-thread workgroups per CU, as the stride-1
//       kernel) and 38 + 48 = 86 KB for BN = 128 (one 512-thread workgroup per CU).  A wave is then one 32-pixel row x 64
//       channels (MI = 2): 6 fragment reads per 8 MFMAs where the stride-1 kernel has 8 per 16.
//   (b) input gradient, S = 1, NTAPS = 1 / 2 / 4: one parity class (py, px) of the stride-2 conv's input gradient is a unit-stride
//       conv over dy with 1, 2, 2 or 4 taps at offsets in {0, +1}, written at out_sy = out_sx = 2, out_oy = py, out_ox = px.  8 x 32
//       tiles, the image is the 9 x 33 window; the (0,1)(2,3)... interval pairing becomes 1, 1 and 2 intervals per chunk.  The
//       pack is ssg_pack_weights_bf16x1_taps of rows [c_lo, c_hi) of the transposed kmode-0 matrix for the class's taps.
// Barrier intervals: taps (2 iv, 2 iv + 1) of a chunk share one barrier and one ring stage; the last interval of an odd tap count
// has one step, its second DMA piece issued with every lane out of range so that vmcnt stays uniform.  In interval 0 the NEXT
// chunk's pixel loads are issued BEFORE the weight pieces of interval + 2, so at the top of every interval "all but the newest
// pieces" (plus the pixel loads issued one interval ago, where a chunk has more than one interval) covers what the interval needs.
#include "common.h"
#include "lds_dma.h"
#include "conv_k32_bf16_host.h"
#include "mfma_split.h"
#include "conv_k32_tail.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int S>
struct Geo {
  static constexpr int TH = S == 2 ? 4 : 8, TW = 32;
  static constexpr int ORG = S == 2 ? 1 : 0;               // tap offsets are dy + ORG in [0, EXT)
  static constexpr int EXT = S == 2 ? 3 : 2;
  static constexpr int HW = (TW - 1) * S + EXT, HH = (TH - 1) * S + EXT, HR = HW * HH;
  static constexpr int PL = (HW + 1) / 2;                  // S = 2: odd-column plane of a row starts here
  static constexpr int NPIX = (HR + 15) / 16 * 16;
  static constexpr int KGS = NPIX * 16 + 64;               // bytes between k-groups: + 64 B, as conv_halo_k32_bf16.hip
  static constexpr int IMG = (4 * KGS + 1023) / 1024 * 1024;
  static constexpr int lds_bytes(int BN) { return IMG + 3 * 2 * BN * 64; }
  // slot of window pixel (wy, wx) in a k-group's plane
  __host__ __device__ static constexpr int col(int wx) { return S == 2 ? (wx & 1) * PL + (wx >> 1) : wx; }
};

template <int BN, int WAVES_N, int NTAPS, int S>
__global__ __launch_bounds__(4 * WAVES_N * 64, 2) void conv_s2_k32_x1_kernel(const ConvArgs a) {
  typedef Geo<S> G;
  constexpr int WAVES_M = 4, NW = WAVES_M * WAVES_N, NT = NW * 64;
  constexpr int TH = G::TH, TW = G::TW, HW = G::HW, HR = G::HR, KGS = G::KGS, IMG = G::IMG, ORG = G::ORG;
  constexpr int BSTG = BN * 64;                          // bytes of one step's weights (one tap x 32 channels)
  constexpr int STG = 2 * BSTG;                          // a ring stage: two steps
  constexpr int B_PC = STG / 1024 / NW;                  // DMA pieces per wave and interval
  constexpr int WTM = TH * TW / WAVES_M, WTN = BN / WAVES_N;
  constexpr int MI = WTM / 16, NI = WTN / 16;
  constexpr int NGRP = (HR + 7) / 8, GPW = (NGRP + NW - 1) / NW, NLD = GPW;
  constexpr int NIV = (NTAPS + 1) / 2;                   // barrier intervals per chunk
  constexpr bool EARLY_CV = NIV >= 3;                    // the prefetched pixels have landed by the top of interval 2: convert behind the last MFMAs
  static_assert(STG % (1024 * NW) == 0 && B_PC == 2 && BSTG == NW * 1024, "two whole 1-KiB pieces per wave and interval; piece j of a wave lies in step + j");
  static_assert(WTN == 64 && WTM % 32 == 0, "a wave owns whole 32-pixel tile rows x 64 channels");
  static_assert(IMG % 1024 == 0, "the ring behind the image stays 1-KiB aligned");
  static_assert(NI * 4 * NT * 4 <= G::lds_bytes(BN), "the slow path's scratch (one accumulator row group per thread) fits the LDS allocation");
  static_assert(NTAPS == 1 || NTAPS == 2 || NTAPS == 4 || NTAPS == 9, "tap counts of the stride-2 forward and of its parity classes");

  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  unsigned char* const img = lds;
  unsigned char* const ring = lds + IMG;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int l15 = lane & 15, kg = lane >> 4;

  const ConvTile tile = ssg_conv_tile(a);
  const int nyt = a.ntiles_n, nt = tile.nt, n0 = nt * BN, tx = tile.tx, ty = tile.ty, n = tile.n;

  const int nchunks = a.C1 >> 5;
  const int nsteps = nchunks * NTAPS;
  const unsigned OOB = 0xffffffffu;
  const unsigned npix = (unsigned)a.N * (unsigned)a.H * (unsigned)a.W;
  const auto in1_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in1), 0, (int)(npix * (unsigned)a.ld1 * 4u), 0x00020000);
  const auto w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)((unsigned)nyt * (unsigned)nsteps * (unsigned)BSTG), 0x00020000);
  const unsigned w_tile = (unsigned)nt * (unsigned)nsteps * (unsigned)BSTG;

  // ---- pixel load items of this thread: group (wave * GPW + k) of 8 window pixels; lane = (pixel p8 of the group, 16-byte quarter q8 of the chunk)
  const int p8 = lane >> 3, q8 = lane & 7;
  const int hp0 = wave * GPW * 8 + p8;                   // window pixel (row-major) of item 0; item k: + 8 k
  const int iy0 = ty * TH * S - ORG, ix0 = tx * TW * S - ORG;
  const int pix_base = (n * a.H + iy0) * a.W + ix0;
  const unsigned ld4 = (unsigned)a.ld1 * 4u;
  u32x4 raw[NLD];
  auto load_px = [&](int chunk) {
    const bool live = chunk < nchunks;                   // past the last chunk: out-of-range lanes keep vmcnt uniform, nothing is fetched
    const unsigned so = (unsigned)chunk * 128u;
#pragma unroll
    for (int k = 0; k < GPW; ++k) {
      const int hp = hp0 + 8 * k;
      const int hy = hp / HW, hx = hp - hy * HW;
      const bool ok = live && hp < HR && (unsigned)(iy0 + hy) < (unsigned)a.H && (unsigned)(ix0 + hx) < (unsigned)a.W;
      const unsigned vo = ok ? (unsigned)(pix_base + hy * a.W + hx) * ld4 + (unsigned)q8 * 16u : OOB;
      raw[k] = __builtin_amdgcn_raw_buffer_load_b128(in1_rs, vo, live ? so : 0u, 0);
    }
  };
  bf16x4 cv[GPW];
  auto convert_px = [&]() {
#pragma unroll
    for (int k = 0; k < GPW; ++k) {
      const f32x4 v = __builtin_bit_cast(f32x4, raw[k]);
#pragma unroll
      for (int e = 0; e < 4; ++e) cv[k][e] = (__bf16)v[e];               // round to nearest even; NaN stays NaN, |x| >= 2^128 - 2^119 becomes inf
    }
  };
  auto write_px = [&]() {
#pragma unroll
    for (int k = 0; k < GPW; ++k) {
      const int hp = hp0 + 8 * k;
      const int hy = hp / HW, hx = hp - hy * HW;
      if (hp < HR) *(bf16x4*)(img + (q8 >> 1) * KGS + (hy * HW + G::col(hx)) * 16 + (q8 & 1) * 8) = cv[k];
    }
  };
  // the two steps from `step` on (`single`: only the first) -> ring stage `stg`.  Piece j of a wave lies in step + j (a step is NW pieces).
  // A piece that is not wanted -- the second of a single-step interval, both past the last step -- is issued with every lane out of
  // range (the range check is on the VECTOR offset): nothing is fetched, vmcnt stays uniform.
  auto issue_b = [&](int step, int stg, bool single) {
    unsigned char* st = ring + stg * STG;
#pragma unroll
    for (int j = 0; j < B_PC; ++j) {
      const bool ok = step < nsteps && !(single && j == 1);
      const unsigned vo = ok ? (unsigned)lane * 16u : OOB;
      const unsigned so = ok ? w_tile + (unsigned)(step + j) * (unsigned)BSTG + (unsigned)wave * 1024u : 0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (ssg_lds_void*)(st + (wave + NW * j) * 1024), 16, vo, so, 0, 0);
    }
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int pb[MI];                                            // byte offset of this lane's pixel in the image at window offset (0, 0)
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int p = wm * WTM + i * 16 + l15;
    pb[i] = kg * KGS + ((p >> 5) * S * HW + (p & 31)) * 16;   // S = 2: column 2 px + kx is plane slot px + col(kx)
  }
  const int wfrag = wn * NI * 1024 + lane * 16;          // this lane's 16 bytes of fragment (wn * NI + j) of a step: + j * 1024

  // ---- prologue: pixels of chunk 0 (the oldest vmcnt entries), two weight intervals in flight
  constexpr bool SINGLE_LAST = (NTAPS & 1) != 0;         // the last interval of a chunk holds one step
  load_px(0);
  issue_b(0, 0, NIV == 1 && SINGLE_LAST);
  if (NIV > 1) issue_b(2, 1, NIV == 2 && SINGLE_LAST);
  else issue_b(NTAPS, 1, SINGLE_LAST);
  wait_vmcnt<2 * B_PC>();
  convert_px();
  write_px();

  int stg = 0;                                           // ring stage of the current interval
  for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma unroll
    for (int iv = 0; iv < NIV; ++iv) {
      // newest first: the weight pieces of the next interval, then (iv == 1) the pixel loads issued in interval 0
      if (iv == 1) wait_vmcnt<B_PC + NLD>();
      else wait_vmcnt<B_PC>();
      wait_lds_reads();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (iv == 0 && chunk > 0) {
        // every wave has left the last tap of the previous chunk: replace the image
        if (!EARLY_CV) convert_px();
        write_px();
        wait_lds_reads();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      const unsigned char* st = ring + stg * STG + wfrag;
      const int stg2 = stg == 0 ? 2 : stg - 1;             // (stg + 2) % 3: the stage every wave left at the barrier above
      // interval iv + 2, counted on into the following chunks
      const int dchunk = (iv + 2) / NIV, iv2 = (iv + 2) % NIV;
      const int nstep = (chunk + dchunk) * NTAPS + 2 * iv2;
      const bool single2 = SINGLE_LAST && iv2 == NIV - 1;
      const int NH = (SINGLE_LAST && iv == NIV - 1) ? 1 : 2;
      bf16x8 p[2][MI], w[2][NI];
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const int tb = (int)((a.tap_bits >> (6 * (2 * iv + h))) & 63ull);    // ssg_tap_dy / ssg_tap_dx (common.h) written out
        const int ky = (tb & 7) - 2 + ORG, kx = (tb >> 3) - 2 + ORG;
        const int toff = (ky * HW + G::col(kx)) * 16;
#pragma unroll
        for (int i = 0; i < MI; ++i) p[h][i] = *(const bf16x8*)(img + pb[i] + toff);
#pragma unroll
        for (int j = 0; j < NI; ++j) w[h][j] = *(const bf16x8*)(st + h * BSTG + j * 1024);
      }
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        if (h == 0) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int i = 0; i < MI; ++i) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[h][j], p[h][i], acc[i][j], 0, 0, 0);
            if (h == 0 && j == NI / 2 - 1 && i == MI - 1) {
              // the next chunk's pixel loads and the DMA pieces go out among the MFMAs, not into the burst of fragment reads behind the barrier
              __builtin_amdgcn_sched_barrier(0);
              if (iv == 0) load_px(chunk + 1);
              issue_b(nstep, stg2, single2);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
      }
      __builtin_amdgcn_s_setprio(0);
      if (EARLY_CV && iv == NIV - 1) {
        __builtin_amdgcn_sched_barrier(0);
        convert_px();
      }
      stg = stg == 2 ? 0 : stg + 1;
    }
  }
  wait_vmcnt<0>();
  wait_lds_reads();

  // ---- the tail (conv_k32_tail.h): non-finite recompute over the NTAPS taps, then bias / activation / store.  Grid pixel (gy, gx)
  // is output pixel (gy * out_sy + out_oy, gx * out_sx + out_ox); the descriptor check refuses a residual, so a.res is null.
  ssg_k32_recompute_nonfinite<NTAPS, TH, WTM, WTN, NT>(acc, lds, tid, n, ty, tx, n0, wm, wn, kg, l15);
  ssg_k32_epilogue<TH, WTM, WTN>(a, acc, n, ty, tx, n0, wm, wn, kg, l15);
}

template <int BN, int WAVES_N, int NTAPS, int S>
int launch(const ConvArgs& a0, hipStream_t st) {
  ConvArgs a = a0;
  const dim3 grid = ssg_conv_tile_grid(a, Geo<S>::TW, Geo<S>::TH, BN);
  constexpr int lds_bytes = Geo<S>::lds_bytes(BN);
  static_assert((BN == 64 ? 2 : 1) * lds_bytes <= 160 * 1024, "LDS: two 256-thread workgroups per CU for BN = 64, one 512-thread workgroup for BN = 128");
  SSG_DYN_LDS_ONCE((conv_s2_k32_x1_kernel<BN, WAVES_N, NTAPS, S>), lds_bytes, "conv bf16x1 s2");
  hipLaunchKernelGGL((conv_s2_k32_x1_kernel<BN, WAVES_N, NTAPS, S>), grid, dim3(4 * WAVES_N * 64), lds_bytes, st, a);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

// ---- host side: the descriptor checks and the launch sequence are conv_k32_bf16_host.h's (forms K32_S2_FWD: the nine row-major
// taps, input stride 2, unit output stride; K32_S2_CLS: a parity class of the input gradient, unit input stride, 1 / 2 / 4 taps at
// offsets {0, +1}, output stride 2); here the choice of the kernel
template <int NTAPS, int S>
int launch_bn(const ConvArgs& a, hipStream_t st) {
  if (ssg_k32_bf16_bn(a.Cout) == 128) return launch<128, 2, NTAPS, S>(a, st);
  return launch<64, 1, NTAPS, S>(a, st);
}

constexpr const char* FWD = "bf16x1 s2";
constexpr const char* CLS = "bf16x1 cls";

}  // namespace

// Pack format code (1128 / 1064) the stride-2 forward launch for `d` reads (ssg_pack_weights_bf16x1), or 0 where it refuses `d`.
extern "C" int ssg_conv2d_bf16x1_s2_ok(const ssg_conv_desc* d) { return ssg_k32_bf16_conv_fmt(d, K32_S2_FWD, FWD, 1); }

extern "C" int ssg_conv2d_bf16x1_s2_kernel_id(const ssg_conv_desc* d) {
  const int fmt = ssg_conv2d_bf16x1_s2_ok(d);
  return fmt == 1128 ? 73 : fmt == 1064 ? 74 : SSG_EINVAL;
}

extern "C" int ssg_conv2d_bf16x1_s2_f32(const ssg_conv_desc* d, const void* w_bf16x1, void* stream) {
  return ssg_k32_bf16_conv_run(d, w_bf16x1, K32_S2_FWD, FWD, 1, stream, [](const ConvArgs& a, hipStream_t st) { return launch_bn<9, 2>(a, st); });
}

// The same for one parity class of the input gradient (pack: ssg_pack_weights_bf16x1_taps with d->ntaps).
extern "C" int ssg_conv2d_bf16x1_cls_ok(const ssg_conv_desc* d) { return ssg_k32_bf16_conv_fmt(d, K32_S2_CLS, CLS, 1); }

extern "C" int ssg_conv2d_bf16x1_cls_kernel_id(const ssg_conv_desc* d) {
  const int fmt = ssg_conv2d_bf16x1_cls_ok(d);
  if (!fmt) return SSG_EINVAL;
  return 75 + (d->ntaps == 1 ? 0 : d->ntaps == 2 ? 2 : 4) + (fmt == 1128 ? 0 : 1);
}

extern "C" int ssg_conv2d_bf16x1_cls_f32(const ssg_conv_desc* d, const void* w_bf16x1, void* stream) {
  return ssg_k32_bf16_conv_run(d, w_bf16x1, K32_S2_CLS, CLS, 1, stream, [](const ConvArgs& a, hipStream_t st) {
    if (a.ntaps == 1) return launch_bn<1, 1>(a, st);
    if (a.ntaps == 2) return launch_bn<2, 1>(a, st);
    return launch_bn<4, 1>(a, st);
  });
}
