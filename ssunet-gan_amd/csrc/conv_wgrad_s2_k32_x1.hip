// Weight gradient of 3x3 STRIDE-2 pad-1 convolutions, ONE-TERM form on v_mfma_f32_16x16x32_bf16 (opt-in: precision 'bf16x1' with
// wgrad_s2 'bf16x1').  dW[ky][kx][ci][co] = sum over n, oy, ox of x[n, 2oy + ky - 1, 2ox + kx - 1, ci] * dy[n, oy, ox, co].
// The contract and data flow of wgrad_k32_x1_kernel (conv_wgrad_k32_bf16.hip): fp32 NHWC tensors in HBM, both operands rounded ONCE
// to bf16 on the way into LDS ((__bf16)v, round to nearest even), one MFMA per product with fp32 accumulation, dy as the A operand,
// fragments by ds_read_b64_tr_b16 from [pixel][64 channels] planes of 128-byte rows with the chunk XOR keyed by pixel bits 1 and 3,
// split-K slabs [split][tap * Cin + ci][Cout] reduced in order by wgrad_reduce_kernel, OIHW output, the non-finite guard of
// conv_slow.h.  An APPROXIMATION (relative operand error 2^-9 each): ssg_conv2d_wgrad_f32 and ssg_conv2d_wgrad_bf16x1_f32 never
// route here, the caller asks through ssg_conv2d_wgrad_bf16x1_s2_f32.
// What stride 2 changes:
//   * a K-step is 32 OUTPUT pixels ox0 .. ox0 + 31 of one output row oy; steps walk down a 32-output-column strip.  The step reads
//     x rows 2oy - 1, 2oy, 2oy + 1 at columns 2ox0 - 1 .. 2ox0 + 63, every second column per tap -- which a transposed read cannot
//     gather.  So an x row is staged as TWO planes by column parity: E[j] = x[2(ox0 + j)], j = 0..31, and O[j] = x[2(ox0 + j) - 1],
//     j = 0..32.  Taps kx = 0, 1, 2 read O[j], E[j], O[j + 1]: 32 contiguous pixel rows each, the read side of the stride-1 kernel.
//     The split is made by the staging address (a thread loads one E piece and one O piece), as conv_s2_k32_x1_kernel's.
//   * consecutive output rows share ONE x row (2oy + 1), so the window rolls by two new x rows per output row.  A barrier interval
//     is one output row: it reads x rows 2oy - 1 .. 2oy + 1 and stages 2oy + 2, 2oy + 3 and dy row oy + 1, loaded at the top of the
//     interval and written after its MFMAs.  x row r sits in slot (r + 1) & 7 (3 read + 2 written of 8), dy row r in slot r & 3.
//   * out-of-image rows and columns (row -1, column -1, column W for odd W, row H for odd H) read as zero through the buffer
//     descriptor's range check.
// Tile: 9 taps x 64 input channels x 128 output channels where Cout % 128 == 0 (NJ = 4), x 64 elsewhere (NJ = 2); a wave = 16 input
// channels x 9 taps x NJ output-channel fragments, 9 * NJ MFMAs and 2 * NJ + 18 transposed reads per step.
// LDS: x 8 slots x (36 + 32) pixel rows x 128 B = 68 KB, dy 4 slots x (NJ / 2) x 32 x 128 B = 16 / 32 KB.
// Legal shapes (ssg_conv2d_wgrad_bf16x1_s2_ok): the nine row-major taps of the 3x3 window, in_sy = in_sx = 2, pad 1, GH = (H + 1) / 2,
// GW = (W + 1) / 2, GW >= 17, C1 % 64 == 0, C2 == 0, Cout % 64 == 0, pixel strides multiples of 4, tensors within 32-bit byte
// offsets, no in_scale.
#include "common.h"
#include "lds_dma.h"
#include "conv_k32_bf16_host.h"
#include "mfma_split.h"
#include "conv_slow.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int KP = WG_BF16_KP;             // output pixels per K-step
constexpr int OPX = 36;                    // pixel rows of the odd-column plane (33 used: O[0] .. O[32])
constexpr int EOFF = OPX * 128;            // the even-column plane (32 pixel rows) follows it
constexpr int XSLOT = (OPX + KP) * 128;    // bytes of one staged x row
constexpr int XSLOTS = 8;
constexpr int XIMG = XSLOTS * XSLOT;
constexpr int DHALF = KP * 128;            // one dy row, 64 output channels
constexpr int DSLOTS = 4;
constexpr int CB = WG_BF16_CB;
constexpr int s2_lds_bytes(int NJ) { return XIMG + DSLOTS * (NJ / 2) * DHALF; }

// 16-byte chunk c (0..7) of pixel row p sits at chunk position c ^ sw(p)
__device__ __forceinline__ int sw(int p) { return ((((p >> 1) & 1) | (((p >> 3) & 1) << 1)) << 1); }

template <int NJ>
__global__ __launch_bounds__(512, 1) void wgrad_s2_k32_x1_kernel(const WgArgs a) {
  constexpr int NH = NJ / 2;                             // 64-channel halves of a dy row
  constexpr int BN = 32 * NJ;
  constexpr int DSLOT = NH * DHALF;
  static_assert(NJ == 2 || NJ == 4, "64 or 128 output channels per workgroup");
  static_assert(s2_lds_bytes(NJ) <= 160 * 1024, "one workgroup per CU within the 160 KB of LDS");
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  unsigned char* const ximg = lds;
  unsigned char* const dimg = lds + XIMG;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;               // 16-channel block of the 64, group of NJ output-channel fragments
  const int l15 = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * CB, n0 = blockIdx.y * BN;
  const int Cin = a.C1;
  const int XB = (a.GW + KP - 1) / KP;

  // ---- this workgroup's range of K-steps, S = strip * GH + oy (strip = image * XB + output-column strip)
  const long long total = (long long)a.N * XB * a.GH;
  long long S0 = (long long)blockIdx.z * a.steps_per_split, S1 = S0 + a.steps_per_split;
  if (S1 > total) S1 = total;

  const unsigned OOB = 0xffffffffu;
  const unsigned npix = (unsigned)a.N * (unsigned)a.H * (unsigned)a.W;
  const auto x_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in1), 0, (int)(npix * (unsigned)a.ld1 * 4u), 0x00020000);
  const auto d_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dout), 0, (int)((unsigned)a.N * (unsigned)a.GH * (unsigned)a.GW * (unsigned)a.ldd * 4u), 0x00020000);

  // ---- staging items, 16-byte pieces in lane order: every thread moves piece (pixel j = tid >> 4, quarter tid & 15) of the even
  // plane, of the odd plane, and of each 64-channel half of a dy row; threads 0..15 also move O[32].  A piece outside the image
  // reads zeros through the descriptor's range check.
  const int s_px = tid >> 4, s_q = tid & 15;
  const bool has_x2 = tid < 16;
  const int x_dst = s_px * 128 + (((s_q >> 1) ^ sw(s_px)) << 4) + (s_q & 1) * 8;
  const int x_dst2 = 32 * 128 + (((s_q >> 1) ^ sw(32)) << 4) + (s_q & 1) * 8;
  const int d_dst = x_dst;                               // same (pixel, quarter) position in a dy half

  struct RawX { u32x4 e, o, o2; };
  struct RawD { u32x4 h[NH]; };
  auto load_x = [&](int n, int row, int ox0) -> RawX {   // x row `row` (may be -1 or >= H: zeros), columns 2 ox0 - 1 .. 2 ox0 + 63
    const bool rin = (unsigned)row < (unsigned)a.H;
    const int ce = 2 * (ox0 + s_px);                     // E[s_px]; O[s_px] is the column before it, O[32] is column 2 ox0 + 63
    const unsigned rowbase = (unsigned)((n * a.H + row) * a.W);
    const unsigned cho = (unsigned)(c0 + 4 * s_q) * 4u;
    const unsigned ve = (rin && ce < a.W) ? (rowbase + (unsigned)ce) * (unsigned)a.ld1 * 4u + cho : OOB;
    const unsigned vo = (rin && ce >= 1 && ce - 1 < a.W) ? (rowbase + (unsigned)(ce - 1)) * (unsigned)a.ld1 * 4u + cho : OOB;
    const int c2 = 2 * ox0 + 63;
    const unsigned vo2 = (has_x2 && rin && c2 < a.W) ? (rowbase + (unsigned)c2) * (unsigned)a.ld1 * 4u + cho : OOB;
    RawX r;
    r.e = __builtin_amdgcn_raw_buffer_load_b128(x_rs, ve, 0, 0);
    r.o = __builtin_amdgcn_raw_buffer_load_b128(x_rs, vo, 0, 0);
    r.o2 = __builtin_amdgcn_raw_buffer_load_b128(x_rs, vo2, 0, 0);
    return r;
  };
  auto load_d = [&](int n, int oy, int ox0) -> RawD {
    const int ox = ox0 + s_px;
    const bool ok = oy < a.GH && ox < a.GW;
    RawD r;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const unsigned vo = ok ? (unsigned)((n * a.GH + oy) * a.GW + ox) * (unsigned)a.ldd * 4u + (unsigned)(n0 + 64 * h + 4 * s_q) * 4u : OOB;
      r.h[h] = __builtin_amdgcn_raw_buffer_load_b128(d_rs, vo, 0, 0);
    }
    return r;
  };
  auto put = [&](unsigned char* dst, u32x4 raw) {
    const f32x4 v = __builtin_bit_cast(f32x4, raw);
    bf16x4 p;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = (__bf16)v[e];     // round to nearest even; NaN stays NaN, |v| >= 2^128 - 2^119 becomes inf
    *(bf16x4*)dst = p;
  };
  auto store_x = [&](const RawX& r, int slot) {
    unsigned char* const s = ximg + slot * XSLOT;
    put(s + EOFF + x_dst, r.e);
    put(s + x_dst, r.o);
    if (has_x2) put(s + x_dst2, r.o2);
  };
  auto store_d = [&](const RawD& r, int slot) {
#pragma unroll
    for (int h = 0; h < NH; ++h) put(dimg + slot * DSLOT + h * DHALF + d_dst, r.h[h]);
  };

  // ---- transposed-read addresses.  Operand k-group g covers pixels 8g .. 8g+7 of the step; lane 4q+pp of the group supplies pixel
  // row q (t adds 4), channels 4pp .. 4pp+3 of the 16-channel block.  Tap kx reads O[j], E[j], O[j + 1].
  const int q4 = l15 >> 2, pp = l15 & 3;
  int xoff[3][2], doff[NJ][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int j = 8 * g + q4 + 4 * t;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int p = j + (kx >> 1);
      xoff[kx][t] = (kx == 1 ? EOFF : 0) + p * 128 + ((((2 * wm + (pp >> 1)) ^ sw(p))) << 4) + (pp & 1) * 8;
    }
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      const int blk = NJ * wn + jj;                      // 16-channel block of the BN output channels: half blk >> 2, block blk & 3 of it
      doff[jj][t] = (blk >> 2) * DHALF + j * 128 + ((((2 * (blk & 3) + (pp >> 1)) ^ sw(j))) << 4) + (pp & 1) * 8;
    }
  }

  // One accumulator sums a whole slab: the planner keeps a slab at <= WG_BF16_MAX_ROWS K-steps (4096 pixels)
  f32x4 acc[9][NJ];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto frag = [&](const unsigned char* base, int o0, int o1) -> bf16x8 {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + o0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + o1));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
  };

  long long S = S0;
  while (S < S1) {
    // ---- segment: output rows [ga, gb) of one column strip
    const int strip = (int)(S / a.GH), ga = (int)(S - (long long)strip * a.GH);
    long long Se = (long long)(strip + 1) * a.GH;
    if (Se > S1) Se = S1;
    const int gb = ga + (int)(Se - S);
    const int n = strip / XB, ox0 = (strip - n * XB) * KP;

    // prologue: x rows 2ga - 1 .. 2ga + 1 and dy row ga.  x row r sits in slot (r + 1) & 7, dy row r in slot r & 3.
    wait_lds_reads();
    __builtin_amdgcn_s_barrier();                        // the previous segment's last reads are done
    asm volatile("" ::: "memory");
    {
      const RawX r0 = load_x(n, 2 * ga - 1, ox0), r1 = load_x(n, 2 * ga, ox0);
      store_x(r0, (2 * ga) & 7); store_x(r1, (2 * ga + 1) & 7);
    }
    {
      const RawX r2 = load_x(n, 2 * ga + 1, ox0);
      const RawD d0 = load_d(n, ga, ox0);
      store_x(r2, (2 * ga + 2) & 7); store_d(d0, ga & 3);
    }

    for (int oy = ga; oy < gb; ++oy) {
      wait_lds_reads();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const bool more = oy + 1 < gb;
      // the next row's operands (x rows 2oy + 2, 2oy + 3 and dy row oy + 1) are in flight behind this row's MFMAs and are written
      // into slots no wave reads in this interval
      RawX nx0, nx1; RawD nd;
      if (more) { nx0 = load_x(n, 2 * oy + 2, ox0); nx1 = load_x(n, 2 * oy + 3, ox0); nd = load_d(n, oy + 1, ox0); }
      __builtin_amdgcn_s_setprio(1);
      const unsigned char* db = dimg + (oy & 3) * DSLOT;
      bf16x8 df[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) df[j] = frag(db, doff[j][0], doff[j][1]);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const unsigned char* xb = ximg + ((2 * oy + ky) & 7) * XSLOT;       // x row 2oy - 1 + ky -> slot (x row + 1) & 7
        bf16x8 xf[3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) xf[kx] = frag(xb, xoff[kx][0], xoff[kx][1]);
        // A = dy (rows = output channels), B = x (columns = input channels)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[ky * 3 + kx][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[j], xf[kx], acc[ky * 3 + kx][j], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
      if (more) {
        __builtin_amdgcn_sched_barrier(0);
        store_x(nx0, (2 * oy + 3) & 7);
        store_x(nx1, (2 * oy + 4) & 7);
        store_d(nd, (oy + 1) & 3);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    S = Se;
  }

  // ---- slab [split][row = tap * Cin + ci][Cout]: acc[tap][j][r] = (ci = c0 + wm*16 + l15, co = n0 + (NJ*wn + j)*16 + 4g + r)
  float* slab = a.ws + (size_t)blockIdx.z * a.M * a.Cout;
  const int ci = c0 + wm * 16 + l15;
  bool bad = false;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) bad |= ssg_nonfinite(acc[t][j][r]);
  if (ssg_any_nonfinite(bad)) {
    // non-finite operands (conv_slow.h): the tile is recomputed from the fp32 operands.  The values go straight to the slab from a
    // rolled loop, not back into the accumulators (ssg_slow_refill4): the accumulators are dead here, and the refill of
    // wgrad_k32_x1_kernel is what spills 123 registers in its cold path.  in_sy = in_sx = 2: ssg_wgrad_slow_pixel reads x at
    // 2 * (oy, ox) + tap.
    const WgArgs& as = *ssg_reload_args<WgArgs>();
#pragma unroll 1
    for (int e = 0; e < 9 * NJ * 4; ++e) {
      const int t = e / (NJ * 4), j = (e / 4) % NJ, r = e & 3;
      const int co = n0 + (NJ * wn + j) * 16 + 4 * g + r;
      slab[((size_t)t * Cin + ci) * as.Cout + co] = ssg_wgrad_slow_value_strips<false>(as, t, ci, co, S0, S1, KP);
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      *(f32x4*)(slab + ((size_t)t * Cin + ci) * a.Cout + n0 + (NJ * wn + j) * 16 + 4 * g) = acc[t][j];
}

// ---- host side: conv_k32_bf16_host.h at input stride 2; here only the choice of the kernel
template <int NJ>
int s2_launch(const WgArgs& a, dim3 grid, hipStream_t st) {
  constexpr int lds_bytes = s2_lds_bytes(NJ);
  SSG_DYN_LDS_ONCE(wgrad_s2_k32_x1_kernel<NJ>, lds_bytes, "wgrad bf16x1 s2");
  hipLaunchKernelGGL(wgrad_s2_k32_x1_kernel<NJ>, grid, dim3(512), lds_bytes, st, a);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

}  // namespace

extern "C" int ssg_conv2d_wgrad_bf16x1_s2_ok(const ssg_wgrad_desc* d) { return ssg_wgrad_bf16_shape_ok(d, 2) ? 1 : 0; }
extern "C" int ssg_conv2d_wgrad_bf16x1_s2_kernel_id(const ssg_wgrad_desc* d) {
  return ssg_wgrad_bf16_shape_ok(d, 2) ? (d->Cout % 128 == 0 ? 81 : 82) : SSG_EINVAL;
}
extern "C" int64_t ssg_conv2d_wgrad_bf16x1_s2_workspace_bytes(const ssg_wgrad_desc* d) { return ssg_wgrad_bf16_ws_bytes(d, 2); }
extern "C" int ssg_conv2d_wgrad_bf16x1_s2_f32(const ssg_wgrad_desc* d, void* stream) {
  return ssg_wgrad_bf16_run(d, 2, "bf16x1 s2", stream, [](int nj, const WgArgs& a, dim3 grid, hipStream_t st) {
    return nj == 4 ? s2_launch<4>(a, grid, st) : s2_launch<2>(a, grid, st);
  });
}
