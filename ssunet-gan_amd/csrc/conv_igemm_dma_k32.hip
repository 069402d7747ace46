// Split-operand (bf16x3) implicit-GEMM convolution of the LDS-DMA family, split-once body on v_mfma_f32_16x16x32_bf16.  Same ConvArgs,
// tile map (8 x 16 pixels x BN output channels, ssg_conv_tile), split pack, bnpart rows and arithmetic (mfma_split.h: three bf16
// terms, the six products small terms first, fp32 accumulation) as conv_igemm_dma_x3_kernel (conv_igemm_dma_x3.hip), which it
// replaces wherever ssg_conv_dma_k32_ok holds.  What differs, after conv_wgrad_dma_k32.hip and conv_igemm_halo_k32.hip:
//   * a K-step is 32 channels of one tap.  The pack stays [Cout tile][step16][BN rows][96 B]: the step reads the two 16-channel
//     blocks at 16-steps s and s + ntaps (12 / 6 contiguous KiB each) through a two-stage LDS-DMA ring (issued one step ahead, landed before the step's MFMAs start: see the main loop); an odd number of 16-channel
//     chunks leaves the second block of the last chunk out of range: zeros, not a branch;
//   * every activation is loaded and split ONCE per workgroup, on the way from HBM into LDS (buffer loads -> registers -> split3_4 ->
//     three bf16 planes [128 pixels][32 channels]); the old body splits every fragment in the wave that reads it, after each read.
//     The planes are single-buffered, the next step's loads are in flight in registers across the MFMAs;
//   * weights are the A operand: a lane holds four consecutive output channels of one pixel and stores 16 bytes;
//   * 2 x 2 waves of 64 pixels x BN / 2 channels: 96 (48) MFMAs per wave between the barriers.
// K order inside a step.  Lane group g = lane >> 4 of a 16x16x32 operand holds 8 consecutive k; which 8 channels those are is free as
// long as both operands agree.  Here g holds channels 16 * (g & 1) + 8 * (g >> 1) .. + 7 of the step: block g & 1, k-half g >> 1 of the
// pack.  A ds_read_b128 is served in 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+ 32): rows 0-3 and 12-15 with one g and
// rows 4-11 with the next.  With g -> (block g >> 1, half g & 1) the two g of a service group are the two halves of one block, and
// rows 4 and 12 meet on one 16-byte slot (2-way); with this order both g of a service group read the SAME half of two blocks
// (blocks are multiples of 256 B apart), which is the 16-rows-one-half read mfma_split.h lays the rows out for: 16 distinct slots.
// Pixel planes: 64-byte rows, 16-byte slot g of pixel p at position g ^ sw(p), sw(p) = 3 * bit 3 of p ^ bit 1 of p: the four pixels
// p, p + 4, p + 8, p + 12 that share a 64-byte phase of the 256-byte bank row read four distinct slots in each service group, and the
// 16 contiguous lanes of a ds_write_b64 group (4 pixels x 2 slots x 2 halves) cover 128 distinct bytes mod 128.
#include "common.h"
#include "lds_dma.h"
#include "conv_args.h"
#include "mfma_split.h"
#include "conv_slow.h"

int ssg_conv_dma_x3_bn(const ConvArgs& a);

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int APL = 128 * 64;              // one bf16 plane of the pixel tile: [128 pixels][32 channels]
constexpr int AIMG = 3 * APL;
constexpr int WSTAGES = 2;

__device__ __forceinline__ int px_sw(int p) { return (3 * ((p >> 3) & 1)) ^ ((p >> 1) & 1); }

template <int BN>
__global__ __launch_bounds__(256, 2) void conv_igemm_dma_x3_k32_kernel(const ConvArgs a) {
  constexpr int TH = 8;
  constexpr int NJ = BN / 32;              // 16-channel fragments per wave: 4 / 2
  constexpr int BSTG = BN * XROW;          // one 16-channel block of the pack
  constexpr int WSTG = 2 * BSTG;           // the two blocks of a 32-channel step
  constexpr int BPIECES = WSTG / 1024;     // 24 / 12 DMA pieces per step
  constexpr int B_PC = BPIECES / 4;        // per wave: 6 / 3
  static_assert(BPIECES % 4 == 0, "whole pieces per wave");

  extern __shared__ __attribute__((aligned(1024))) unsigned char ldsb[];     // AIMG + WSTAGES * WSTG bytes

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, kg = lane >> 4;

  const ConvTile tile = ssg_conv_tile(a);
  const int nyt = a.ntiles_n, nt = tile.nt, n0 = nt * BN, tx = tile.tx, ty = tile.ty, n = tile.n;

  const int ntaps = a.ntaps;
  const int nsteps16 = a.nsteps;
  const int nchunk16 = nsteps16 / ntaps;
  const int nsteps = ((nchunk16 + 1) >> 1) * ntaps;      // 32-channel steps
  const int Cin = a.C1 + a.C2;

  const unsigned OOB = 0xffffffffu;
  const unsigned npix = (unsigned)a.N * (unsigned)a.H * (unsigned)a.W;
  const auto in1_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in1), 0, (int)(npix * (unsigned)a.ld1 * 4u), 0x00020000);
  const auto in2_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in2), 0, (int)(npix * (unsigned)a.ld2 * 4u), 0x00020000);
  const auto w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)((unsigned)nyt * (unsigned)nsteps16 * (unsigned)BSTG), 0x00020000);

  // ---- activation pieces: this thread's channel quad q4 of both 16-channel halves at tile pixels a_p and a_p + 64
  const int a_p = tid >> 2, q4 = tid & 3;
  int a_iy0[2], a_ix0[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int r = a_p + 64 * jj;
    const int gy = ty * TH + (r >> 4), gx = tx * 16 + (r & 15);
    const bool ok = (gy < a.GH) && (gx < a.GW);
    a_iy0[jj] = ok ? gy * a.in_sy : -100000;
    a_ix0[jj] = gx * a.in_sx;
  }
  const unsigned a_q = 16u * (unsigned)q4;
  // plane 0 byte of piece (jj, h): pixel row, slot (h + 2 * (q4 >> 1)) ^ sw, quad half (px_sw(p + 64) = px_sw(p))
  const int a_dst0 = a_p * 64 + 16 * ((0 + 2 * (q4 >> 1)) ^ px_sw(a_p)) + 8 * (q4 & 1);
  const int a_dst1 = a_p * 64 + 16 * ((1 + 2 * (q4 >> 1)) ^ px_sw(a_p)) + 8 * (q4 & 1);

  struct Raw { u32x4 x[4]; };
  int a_c32 = 0, a_t = 0;                                // the step the next load() fetches
  auto load = [&](Raw& r) {
    const int dy = ssg_tap_dy(a.tap_bits, a_t), dx = ssg_tap_dx(a.tap_bits, a_t);
    unsigned vo[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int iy = a_iy0[jj] + dy, ix = a_ix0[jj] + dx;
      const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      vo[jj] = ok ? (unsigned)((n * a.H + iy) * a.W + ix) : OOB;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c0 = a_c32 * 32 + 16 * h;
      const bool valid = c0 < Cin;                       // the second half of an odd last chunk: zeros
      const bool first = c0 < a.C1;                      // C1 % 16 == 0: a 16-channel half lies in one input, uniformly for the wave
      const unsigned ldb = (unsigned)(first ? a.ld1 : a.ld2) * 4u;
      const int so = valid ? (first ? c0 : c0 - a.C1) * 4 : 0;
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const unsigned off = (valid && vo[jj] != OOB) ? vo[jj] * ldb + a_q : OOB;
        if (first) r.x[2 * jj + h] = __builtin_amdgcn_raw_buffer_load_b128(in1_rs, off, so, 0);
        else r.x[2 * jj + h] = __builtin_amdgcn_raw_buffer_load_b128(in2_rs, off, so, 0);
      }
    }
    if (++a_t == ntaps) { a_t = 0; ++a_c32; }
  };
  auto put = [&](unsigned char* base, u32x4 raw) {
    bf16x4 p1, p2, p3;
    split3_4(__builtin_bit_cast(f32x4, raw), p1, p2, p3);
    *(bf16x4*)base = p1; *(bf16x4*)(base + APL) = p2; *(bf16x4*)(base + 2 * APL) = p3;
  };
  auto store = [&](const Raw& r) {
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      put(ldsb + a_dst0 + jj * 64 * 64, r.x[2 * jj + 0]);
      put(ldsb + a_dst1 + jj * 64 * 64, r.x[2 * jj + 1]);
    }
  };

  // ---- weight ring: step S = (chunk32, tap) -> 16-steps (2 * chunk32) * ntaps + tap and + ntaps, BPIECES 1-KiB pieces, B_PC per wave
  const unsigned w_lane = (unsigned)lane * 16u;
  const unsigned w_tile = (unsigned)nt * (unsigned)nsteps16 * (unsigned)BSTG;
  int w_c32 = 0, w_t = 0, w_stage = 0;                   // the step the next wdma() fetches, and its stage
  auto wdma = [&]() {
    unsigned char* st = ldsb + AIMG + w_stage * WSTG;
    const int s16 = 2 * w_c32 * ntaps + w_t;
    const bool second = 2 * w_c32 + 1 < nchunk16;
#pragma unroll
    for (int j = 0; j < B_PC; ++j) {
      const int g = wave + 4 * j;                        // piece g: block g / (BPIECES / 2)
      const bool blk = g >= BPIECES / 2;
      const bool valid = !blk || second;
      const unsigned so = valid ? w_tile + (unsigned)(s16 + (blk ? ntaps : 0)) * (unsigned)BSTG + (unsigned)(g - (blk ? BPIECES / 2 : 0)) * 1024u : 0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (ssg_lds_void*)(st + g * 1024), 16, valid ? w_lane : OOB, so, 0, 0);
    }
    if (++w_t == ntaps) { w_t = 0; ++w_c32; }
    w_stage ^= 1;
  };

  // ---- fragment addresses.  Pixels (B operand): column l15 of pixel group i = tile pixel wm * 64 + i * 16 + l15, k-group kg.
  // Weights (A operand): row l15 of channel group j = tile column wn * (BN / 2) + j * 16 + l15, block kg & 1, k-half kg >> 1
  const int xoff = (wm * 64 + l15) * 64 + 16 * (kg ^ px_sw(l15));
  int woff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int row = wn * (BN / 2) + j * 16 + l15;
    woff[j] = AIMG + (kg & 1) * BSTG + row * XROW + 16 * ((kg >> 1) ^ ((row >> 3) & 1));
  }

  f32x4 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  {
    Raw r;
    wdma();
    load(r);
    if (1 < nsteps) wdma();
    store(r);
  }
  for (int s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;
    // Before the barrier: this step's weights (everything but the next step's B_PC pieces).  After it, on every step but the last,
    // the ring is drained, the next step's pieces (issued at the end of the previous step) included: they land before this step's
    // fragment reads and MFMAs start, and the other workgroup of the CU covers the wait.  The compiler's waitcnt pass put the same
    // drain here on its own account (it cannot see that the two `if (more)` are one condition); it is written out because it is the
    // schedule that was measured and kept: forms that keep the pieces in flight across the MFMAs ran 5-12 % slower on the launches
    // with more than two workgroups per CU.
    if (more) wait_vmcnt<B_PC>();
    else wait_vmcnt<0>();
    wait_lds_reads();
    __builtin_amdgcn_s_barrier();                        // the step's planes are written, its weight stage is whole
    asm volatile("" ::: "memory");
    Raw nx;
    if (more) {
      wait_vmcnt<0>();
      load(nx);
    }

    const unsigned char* const wst = ldsb + (s & 1) * WSTG;
    bf16x8 xf[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 3; ++q) xf[i][q] = *(const bf16x8*)(ldsb + q * APL + xoff + i * 1024);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      bf16x8 wf[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) wf[q] = *(const bf16x8*)(wst + woff[j] + 32 * q);
      // small terms first (conv_igemm_dma_x3_kernel's order); A = weights (rows = output channels), B = pixels
#define SSG_CD_TERM(QX, QW)                                                                         \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                    \
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[QW], xf[i][QX], acc[i][j], 0, 0, 0);
      SSG_CD_TERM(2, 0) SSG_CD_TERM(1, 1) SSG_CD_TERM(0, 2)
      SSG_CD_TERM(1, 0) SSG_CD_TERM(0, 1)
      SSG_CD_TERM(0, 0)
#undef SSG_CD_TERM
    }
    if (more) {
      wait_lds_reads();
      __builtin_amdgcn_s_barrier();                      // every wave has read this step's planes and weight stage
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      store(nx);
      if (s + 2 < nsteps) wdma();                        // into the stage just read
    }
  }
  wait_vmcnt<0>();
  wait_lds_reads();

  // acc[i][j][r] = (tile pixel wm * 64 + i * 16 + l15, output channel co0 + j * 16 + r)
  const int co0 = n0 + wn * (BN / 2) + 4 * kg;
  const int gy0 = ty * TH + wm * 4, gx = tx * 16 + l15;
  {                                                      // non-finite operands: conv_slow.h
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) bad |= ssg_nonfinite(acc[i][j][r]);
    if (ssg_any_nonfinite(bad)) {
      const ConvArgs& as = *ssg_reload_args<ConvArgs>();
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          ssg_slow_refill4(acc[i][j], (float*)ldsb + tid, 256, [&](int r) {
            return ssg_conv_slow_value(as, n, gy0 + i, gx, co0 + j * 16 + r, 0, as.ntaps);
          });
    }
  }

  // ---- epilogue, conv_halo_k32_kernel's for this tile: 16-byte stores, batch-norm partial row of the 8 x 16 tile
  const bool want_bn = a.bnpart != nullptr;
  if (want_bn) __syncthreads();                          // planes, ring and slow-path scratch are dead for every wave
  double* const red = (double*)ldsb;                     // [2][2][BN]
  size_t opix[4]; bool pok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gy = gy0 + i;
    pok[i] = gy < a.GH && gx < a.GW;
    opix[i] = (size_t)(n * a.OH + gy * a.out_sy + a.out_oy) * a.OW + gx * a.out_sx + a.out_ox;
  }
  float nvl = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) nvl += pok[i] ? 1.f : 0.f;
  if (want_bn) nvl = ssg_row16_sum(nvl);                 // valid pixels of this wave's 16-lane row group
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int co = co0 + j * 16;                         // Cout % BN == 0: every column quad is whole
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) bv = *(const f32x4*)(a.bias + co);
    if (want_bn) {
      // fp32 sums of deviations from a pivot the 16 lanes share, converted to fp64 sums of the values once per row group and column
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float piv = ssg_row16_sum(acc[0][j][r] + bv[r]) * 0.0625f;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dv = pok[i] ? (acc[i][j][r] + bv[r]) - piv : 0.f;
          s1 += dv; s2 += dv * dv;
        }
        s1 = ssg_row16_sum(s1); s2 = ssg_row16_sum(s2);
        if (l15 == 0) {
          const double c = (double)piv, nn = (double)nvl;
          const int col = wn * (BN / 2) + j * 16 + kg * 4 + r;
          red[(wm * 2 + 0) * BN + col] = (double)s1 + nn * c;
          red[(wm * 2 + 1) * BN + col] = (double)s2 + 2.0 * c * (double)s1 + nn * c * c;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
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
  if (want_bn) {
    __syncthreads();
    if (tid < BN) {
      const double t1 = red[(0 * 2 + 0) * BN + tid] + red[(1 * 2 + 0) * BN + tid];
      const double t2 = red[(0 * 2 + 1) * BN + tid] + red[(1 * 2 + 1) * BN + tid];
      double* dst = a.bnpart + (size_t)((n * a.tiles_y + ty) * a.tiles_x + tx) * 2 * a.Cout;
      dst[n0 + tid] = t1; dst[a.Cout + n0 + tid] = t2;
    }
  }
}

template <int BN>
int launch(const ConvArgs& a0, hipStream_t st) {
  ConvArgs a = a0;
  const dim3 grid = ssg_conv_tile_grid(a, 16, 8, BN);
  constexpr int lds_bytes = AIMG + WSTAGES * 2 * BN * XROW;
  static_assert(lds_bytes <= 80 * 1024, "two workgroups per CU");
  SSG_DYN_LDS_ONCE(conv_igemm_dma_x3_k32_kernel<BN>, lds_bytes, "conv dma k32");
  hipLaunchKernelGGL((conv_igemm_dma_x3_k32_kernel<BN>), grid, dim3(256), lds_bytes, st, a);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

}  // namespace

// The split-once body serves a launch of the family (ssg_conv_dma_x3_bn) that carries its split pack, whose channel counts and
// pixel strides are whole quads and whose tensors are 16-byte aligned (one buffer load / one store = one quad), within 32-bit byte
// offsets (the inputs: ssg_conv_dma_x3_bn; the pack: here).
bool ssg_conv_dma_k32_ok(const ConvArgs& a) {
  const int bn = ssg_conv_dma_x3_bn(a);
  if (!bn || !a.w || !a.w32 || !a.in1 || !a.in2 || !a.out) return false;
  if ((a.C1 & 15) || (a.C2 & 15) || (a.ld1 & 3) || (a.ld2 & 3) || (a.ldo & 3) || (a.Cout % bn)) return false;
  if (!ssg_aligned16(a.in1) || !ssg_aligned16(a.in2) || !ssg_aligned16(a.w) || !ssg_aligned16(a.w32) || !ssg_aligned16(a.out)) return false;
  if (a.bias && !ssg_aligned16(a.bias)) return false;
  if (a.res && (!ssg_aligned16(a.res) || (a.ldr & 3))) return false;
  if (a.ntaps < 1 || a.nsteps % a.ntaps) return false;
  if ((unsigned long long)(a.Cout / bn) * (unsigned long long)a.nsteps * (unsigned long long)(bn * XROW) > 0x7ffffff0ull) return false;
  return true;
}

int ssg_conv_igemm_dma_k32_launch(const ConvArgs& a, int bn, hipStream_t st) {
  return bn == 128 ? launch<128>(a, st) : launch<64>(a, st);
}
