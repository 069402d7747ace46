// Weight gradient of 3x3 stride-1 pad-1 convolutions on v_mfma_f32_16x16x32_bf16 with the operands in bf16, ONE body template
// wgrad_k32_bf16<NJ, TERMS> behind the kernels of the two opt-in precisions: TERMS = 1 is wgrad_k32_x1_kernel<NJ>, 'bf16x1'
// (ops.train_precision('bf16x1')), TERMS = 2 is wgrad_k32_x2_kernel<NJ>, 'bf16x2'.  The contract of wgrad_k32_kernel (conv_wgrad_k32.hip): dW[tap][ci][co] = sum over pixels of x[p + tap][ci] *
// dy[p][co], fp32 tensors in HBM, one or two input pointers (concat), split-K slabs [split][tap * Cin + ci][Cout] reduced in order
// by wgrad_reduce_kernel, OIHW output.  The difference: both operands (the x window and dy) are turned into TERMS bf16 terms ONCE
// on the way into LDS, one plane per term:
//   TERMS = 1  (__bf16)v, round to nearest even; one MFMA per product.  An APPROXIMATION (relative operand error 2^-9 each).
//   TERMS = 2  split2_4 (mfma_split.h): v1 = bf16_rne(v), v2 = bf16_rne(v - v1); a product is three MFMAs in a fixed order, small
//              terms first: x1 * d2, x2 * d1, x1 * d1 (x2 * d2 is dropped): |x d - kept| <= (3 * 2^-16 + 3 * 2^-32) |x d|.  The
//              three terms of an x row run as three sweeps over its 3 * NJ accumulators, so a dependent MFMA is 3 * NJ issues
//              behind.  With the second terms exactly zero the two extra sweeps add zeros: the result is TERMS = 1's.
// ssg_conv2d_wgrad_f32 and its plan never route here: the caller asks through ssg_conv2d_wgrad_bf16x1_f32 / _bf16x2_f32.
// What is kept from the split kernel: the bf16 plane [pixel][64 channels] in 128-byte rows with the chunk XOR keyed by pixel bits
// 1 and 3, fragments by ds_read_b64_tr_b16, a K-step = 32 pixels of one image row, steps walking DOWN a 32-pixel column strip with
// the x window rolling through LDS row slots, dy as the A operand so that a lane stores 4 consecutive output channels.
// What is not: with one plane a step is 18 MFMAs per wave on the 9 x 64 x 64 tile, six times the feed rate per MFMA.  So
//   * a barrier interval covers TWO image rows of the strip (the x window rolls through 8 row slots, two new rows per interval,
//     dy through 4); the next interval's rows are loaded in two halves, each in flight behind one row's MFMAs;
//   * the tile is 9 taps x 64 input channels x 128 output channels where Cout % 128 == 0 (NJ = 4: a wave = 16 input channels x
//     9 taps x 4 output-channel fragments, 36 accumulators, 72 MFMAs and 52 transposed reads per interval and term; a staged x
//     row serves twice the output channels), and 9 x 64 x 64 (NJ = 2) elsewhere.
// LDS per term: x 8 slots x 36 pixels x 128 B = 36 KB, dy 4 slots x (NJ / 2) x 32 x 128 B = 16 / 32 KB; 52 / 68 KB for one term,
// 104 / 136 KB for two, one 512-thread workgroup per CU.  Registers: 36 / 18 accumulators x 4, TERMS x (NJ + 3) fragments x 4, one
// row of staging values.
// The summation order is fixed by (slab, K-step, term) and the slabs are reduced in order: it does not depend on the grid
// beyond the slab plan, which is a function of the shape alone (and the same for both term counts).
// Legal shapes (ssg_conv2d_wgrad_bf16x1_ok, ssg_conv2d_wgrad_bf16x2_ok: one predicate): the nine row-major taps of the 3x3 window
// at unit stride over the whole image (GH == H, GW == W), C1 % 64 == C2 % 64 == 0, Cout % 64 == 0, GW >= 17, pixel strides
// multiples of 4, tensors within 32-bit byte offsets, no in_scale.
// Non-finite operands (conv_slow.h): an fp32 value >= 2^128 - 2^119 rounds to bf16 infinity although the fp32 product is finite;
// inf times anything is inf or NaN, so a workgroup that holds a non-finite accumulator recomputes its tile from the fp32 operands.
// REQUIRED for two terms: an infinite v1 makes v - v1 a NaN, so every workgroup that reads an infinite or bf16-overflowing operand
// holds a non-finite accumulator.
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

constexpr int KP = WG_BF16_KP;             // pixels per K-step
constexpr int WPX = 36;                    // pixel rows per x slot (34 used: window columns gx0 - 1 .. gx0 + 32)
constexpr int XSLOT = WPX * 128;           // bytes
constexpr int XSLOTS = 8;
constexpr int XIMG = XSLOTS * XSLOT;
constexpr int DHALF = KP * 128;            // one dy row, 64 output channels
constexpr int DSLOTS = 4;
constexpr int CB = WG_BF16_CB;
constexpr int lds_bytes_of(int NJ, int TERMS) { return TERMS * (XIMG + DSLOTS * (NJ / 2) * DHALF); }      // one plane of each image per term

// 16-byte chunk c (0..7) of pixel row p sits at chunk position c ^ sw(p)
__device__ __forceinline__ int sw(int p) { return ((((p >> 1) & 1) | (((p >> 3) & 1) << 1)) << 1); }

template <int NJ, int TERMS>
__device__ __forceinline__ void wgrad_k32_bf16(const WgArgs a) {
  constexpr int NH = NJ / 2;                             // 64-channel halves of a dy row
  constexpr int BN = 32 * NJ;
  constexpr int DSLOT = NH * DHALF;
  constexpr int DIMG = DSLOTS * DSLOT;
  static_assert(NJ == 2 || NJ == 4, "64 or 128 output channels per workgroup");
  static_assert(TERMS == 1 || TERMS == 2, "one rounded term, or the two of split2");
  static_assert(4 * 512 * 4 <= lds_bytes_of(NJ, TERMS), "the slow path's scratch (one accumulator per thread) fits the LDS allocation");
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  unsigned char* const ximg = lds;
  unsigned char* const dimg = lds + TERMS * XIMG;        // plane 1 of x at ximg + XIMG, of dy at dimg + DIMG

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;               // 16-channel block of the 64, group of NJ output-channel fragments
  const int l15 = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * CB, n0 = blockIdx.y * BN;
  const int Cin = a.C1 + a.C2;
  const int XB = (a.GW + KP - 1) / KP;

  // ---- this workgroup's range of K-steps, S = strip * GH + gy (strip = image * XB + column strip)
  const long long total = (long long)a.N * XB * a.GH;
  long long S0 = (long long)blockIdx.z * a.steps_per_split, S1 = S0 + a.steps_per_split;
  if (S1 > total) S1 = total;

  const unsigned OOB = 0xffffffffu;
  const bool first = c0 < a.C1;
  const float* xsrc = first ? a.in1 : a.in2;
  const int xld = first ? a.ld1 : a.ld2;
  const int xc0 = first ? c0 : c0 - a.C1;
  const unsigned npix = (unsigned)a.N * (unsigned)a.H * (unsigned)a.W;
  const auto x_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xsrc), 0, (int)(npix * (unsigned)xld * 4u), 0x00020000);
  const auto d_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dout), 0, (int)((unsigned)a.N * (unsigned)a.GH * (unsigned)a.GW * (unsigned)a.ldd * 4u), 0x00020000);

  // ---- staging items, 16-byte pieces in lane order (wgrad_k32_kernel's): piece t of a new x row = (window pixel t >> 4, quarter
  // t & 15) for every thread, pieces 512..543 (window pixels 32, 33) once more for threads 0..31; piece t of each 64-channel half
  // of a dy row for every thread.  Out-of-image pieces read zeros through the descriptor's range check.
  const int s_px = tid >> 4, s_q = tid & 15;
  const bool has_x2 = tid < 32;
  const int x_dst = s_px * 128 + (((s_q >> 1) ^ sw(s_px)) << 4) + (s_q & 1) * 8;
  const int x_dst2 = (32 + s_px) * 128 + (((s_q >> 1) ^ sw(32 + s_px)) << 4) + (s_q & 1) * 8;      // threads 0..31: s_px = 0, 1
  const int d_dst = x_dst;                               // same (pixel, quarter) position in a dy half

  struct RawX { u32x4 a, b; };
  struct RawD { u32x4 h[NH]; };
  auto x_inside = [&](int row, int gx0, int px) -> bool {        // is window pixel px of row `row` inside the image
    return (unsigned)row < (unsigned)a.H && (unsigned)(gx0 - 1 + px) < (unsigned)a.W;
  };
  auto load_x = [&](int n, int row, int gx0) -> RawX {   // window row `row` (may be -1 or >= H: zeros), columns gx0 - 1 .. gx0 + 32
    const unsigned rowbase = (unsigned)((n * a.H + row) * a.W + gx0 - 1);
    const unsigned cho = (unsigned)(xc0 + 4 * s_q) * 4u;
    const unsigned vo = x_inside(row, gx0, s_px) ? (rowbase + (unsigned)s_px) * (unsigned)xld * 4u + cho : OOB;
    const unsigned vo2 = (has_x2 && x_inside(row, gx0, 32 + s_px)) ? (rowbase + 32u + (unsigned)s_px) * (unsigned)xld * 4u + cho : OOB;
    RawX r;
    r.a = __builtin_amdgcn_raw_buffer_load_b128(x_rs, vo, 0, 0);
    r.b = __builtin_amdgcn_raw_buffer_load_b128(x_rs, vo2, 0, 0);
    return r;
  };
  auto load_d = [&](int n, int gy, int gx0) -> RawD {    // row gy (may be >= GH: zeros, never multiplied)
    const int gx = gx0 + s_px;
    const bool ok = gy < a.GH && gx < a.GW;
    RawD r;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const unsigned vo = ok ? (unsigned)((n * a.GH + gy) * a.GW + gx) * (unsigned)a.ldd * 4u + (unsigned)(n0 + 64 * h + 4 * s_q) * 4u : OOB;
      r.h[h] = __builtin_amdgcn_raw_buffer_load_b128(d_rs, vo, 0, 0);
    }
    return r;
  };
  auto put = [&](unsigned char* dst, int plane, u32x4 raw) {      // the terms of four values, `plane` bytes apart
    const f32x4 v = __builtin_bit_cast(f32x4, raw);
    if constexpr (TERMS == 1) {
      bf16x4 p;
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = (__bf16)v[e];   // round to nearest even; NaN stays NaN, |v| >= 2^128 - 2^119 becomes inf
      *(bf16x4*)dst = p;
    } else {
      bf16x4 p1, p2;
      split2_4(v, p1, p2);                               // NaN stays NaN; |v| >= 2^128 - 2^119: p1 = inf, p2 = NaN
      *(bf16x4*)dst = p1;
      *(bf16x4*)(dst + plane) = p2;
    }
  };
  auto store_x = [&](const RawX& r, int slot) {
    put(ximg + slot * XSLOT + x_dst, XIMG, r.a);
    if (has_x2) put(ximg + slot * XSLOT + x_dst2, XIMG, r.b);
  };
  auto store_d = [&](const RawD& r, int slot) {
#pragma unroll
    for (int h = 0; h < NH; ++h) put(dimg + slot * DSLOT + h * DHALF + d_dst, DIMG, r.h[h]);
  };

  // ---- transposed-read addresses.  Operand k-group g covers pixels 8g .. 8g+7 of the step; lane 4q+pp of the group supplies pixel
  // row q (t adds 4), channels 4pp .. 4pp+3 of the 16-channel block
  const int q4 = l15 >> 2, pp = l15 & 3;
  int xoff[3][2], doff[NJ][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int p = dx + 8 * g + q4 + 4 * t;             // window pixel: step pixel + 1 + (dx - 1)
      xoff[dx][t] = p * 128 + ((((2 * wm + (pp >> 1)) ^ sw(p))) << 4) + (pp & 1) * 8;
    }
    const int p = 8 * g + q4 + 4 * t;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int blk = NJ * wn + j;                       // 16-channel block of the BN output channels: half blk >> 2, block blk & 3 of it
      doff[j][t] = (blk >> 2) * DHALF + p * 128 + ((((2 * (blk & 3) + (pp >> 1)) ^ sw(p))) << 4) + (pp & 1) * 8;
    }
  }

  // One accumulator sums a whole slab: the planner keeps a slab at <= WG_BF16_MAX_ROWS K-steps (4096 pixels), as for wgrad_k32_kernel.
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
    // ---- segment: rows [ga, gb) of one column strip
    const int strip = (int)(S / a.GH), ga = (int)(S - (long long)strip * a.GH);
    long long Se = (long long)(strip + 1) * a.GH;
    if (Se > S1) Se = S1;
    const int gb = ga + (int)(Se - S);
    const int n = strip / XB, gx0 = (strip - n * XB) * KP;

    // prologue: x rows ga-1 .. ga+2 and dy rows ga, ga+1.  x row r sits in slot (r + 1) & 7, dy row r in slot r & 3.
    wait_lds_reads();
    __builtin_amdgcn_s_barrier();                        // the previous segment's last reads are done
    asm volatile("" ::: "memory");
    {                                                    // two batches: four rows in flight at once spilled registers
      const RawX r0 = load_x(n, ga - 1, gx0), r1 = load_x(n, ga, gx0);
      const RawD d0 = load_d(n, ga, gx0);
      store_x(r0, (ga + 0) & 7); store_x(r1, (ga + 1) & 7); store_d(d0, ga & 3);
    }
    {
      const RawX r2 = load_x(n, ga + 1, gx0), r3 = load_x(n, ga + 2, gx0);
      const RawD d1 = load_d(n, ga + 1, gx0);
      store_x(r2, (ga + 2) & 7); store_x(r3, (ga + 3) & 7); store_d(d1, (ga + 1) & 3);
    }

    for (int gy = ga; gy < gb; gy += 2) {
      wait_lds_reads();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const bool more = gy + 2 < gb;
      // the next interval's rows (x gy+3, gy+4 and dy gy+2, gy+3) come in two halves, each in flight behind one row of MFMAs and
      // written into slots no wave reads in this interval: one row of staging registers instead of two
      RawX nx; RawD nd;
      if (more) { nx = load_x(n, gy + 3, gx0); nd = load_d(n, gy + 2, gx0); }
      const int nrows = gy + 1 < gb ? 2 : 1;             // a segment with an odd number of rows ends on a one-row interval
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        if (rr < nrows) {
          const int row = gy + rr;
          if (rr == 0) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(1);      // a wave's priority falls as it advances through an interval
          const unsigned char* db = dimg + (row & 3) * DSLOT;
          bf16x8 df[TERMS][NJ];                          // [plane]
#pragma unroll
          for (int h = 0; h < TERMS; ++h)
#pragma unroll
            for (int j = 0; j < NJ; ++j) df[h][j] = frag(db + h * DIMG, doff[j][0], doff[j][1]);
#pragma unroll
          for (int dyi = 0; dyi < 3; ++dyi) {
            const unsigned char* xb = ximg + ((row + dyi) & 7) * XSLOT;     // x row (row - 1 + dyi) -> slot (x row + 1) & 7
            bf16x8 xf[TERMS][3];
#pragma unroll
            for (int h = 0; h < TERMS; ++h)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) xf[h][dx] = frag(xb + h * XIMG, xoff[dx][0], xoff[dx][1]);
            // A = dy (rows = output channels), B = x (columns = input channels).  One term: one sweep, x1 d1.  Two terms: three
            // sweeps, small terms first: x1 d2, x2 d1, x1 d1
#pragma unroll
            for (int t = 0; t < 2 * TERMS - 1; ++t) {
              const int hd = (TERMS == 2 && t == 0) ? 1 : 0, hx = (TERMS == 2 && t == 1) ? 1 : 0;
#pragma unroll
              for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                  acc[dyi * 3 + dx][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[hd][j], xf[hx][dx], acc[dyi * 3 + dx][j], 0, 0, 0);
            }
          }
        }
        if (more) {
          __builtin_amdgcn_sched_barrier(0);
          store_x(nx, (gy + 4 + rr) & 7);
          store_d(nd, (gy + 2 + rr) & 3);
          if (rr == 0) { nx = load_x(n, gy + 4, gx0); nd = load_d(n, gy + 3, gx0); }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
    S = Se;
  }

  wait_lds_reads();
  {                                                      // non-finite operands: conv_slow.h
    bool bad = false;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) bad |= ssg_nonfinite(acc[t][j][r]);
    if (ssg_any_nonfinite(bad)) {
      const WgArgs& as = *ssg_reload_args<WgArgs>();
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          ssg_slow_refill4(acc[t][j], (float*)lds + tid, 512, [&](int r) {
            return ssg_wgrad_slow_value_strips<false>(as, t, c0 + wm * 16 + l15, n0 + (NJ * wn + j) * 16 + 4 * g + r, S0, S1, KP);
          });
    }
  }

  // ---- slab [split][row = tap * Cin + ci][Cout]: acc[tap][j][r] = (ci = c0 + wm*16 + l15, co = n0 + (NJ*wn + j)*16 + 4g + r)
  float* slab = a.ws + (size_t)blockIdx.z * a.M * a.Cout;
  const int ci = c0 + wm * 16 + l15;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      *(f32x4*)(slab + ((size_t)t * Cin + ci) * a.Cout + n0 + (NJ * wn + j) * 16 + 4 * g) = acc[t][j];
}

// The two kernels keep the names their profiling labels and traces have had: one line each over the shared body.
template <int NJ>
__global__ __launch_bounds__(512, 1) void wgrad_k32_x1_kernel(const WgArgs a) { wgrad_k32_bf16<NJ, 1>(a); }
template <int NJ>
__global__ __launch_bounds__(512, 1) void wgrad_k32_x2_kernel(const WgArgs a) { wgrad_k32_bf16<NJ, 2>(a); }

// ---- host side: conv_k32_bf16_host.h, the same for both term counts (the shapes, the slab plan and the workspace do not depend on
// TERMS); here only the choice of the kernel
template <int NJ, int TERMS>
int launch(const WgArgs& a, dim3 grid, hipStream_t st) {
  constexpr int lds_bytes = lds_bytes_of(NJ, TERMS);
  if constexpr (TERMS == 1) {
    SSG_DYN_LDS_ONCE(wgrad_k32_x1_kernel<NJ>, lds_bytes, "wgrad bf16x1");
    hipLaunchKernelGGL(wgrad_k32_x1_kernel<NJ>, grid, dim3(512), lds_bytes, st, a);
  } else {
    SSG_DYN_LDS_ONCE(wgrad_k32_x2_kernel<NJ>, lds_bytes, "wgrad bf16x2");
    hipLaunchKernelGGL(wgrad_k32_x2_kernel<NJ>, grid, dim3(512), lds_bytes, st, a);
  }
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

template <int TERMS>
int run(const ssg_wgrad_desc* d, void* stream) {
  return ssg_wgrad_bf16_run(d, 1, TERMS == 1 ? "bf16x1" : "bf16x2", stream, [](int nj, const WgArgs& a, dim3 grid, hipStream_t st) {
    return nj == 4 ? launch<4, TERMS>(a, grid, st) : launch<2, TERMS>(a, grid, st);
  });
}

}  // namespace

extern "C" int ssg_conv2d_wgrad_bf16x1_ok(const ssg_wgrad_desc* d) { return ssg_wgrad_bf16_shape_ok(d, 1) ? 1 : 0; }
extern "C" int ssg_conv2d_wgrad_bf16x1_kernel_id(const ssg_wgrad_desc* d) { return ssg_wgrad_bf16_shape_ok(d, 1) ? 72 : SSG_EINVAL; }
extern "C" int64_t ssg_conv2d_wgrad_bf16x1_workspace_bytes(const ssg_wgrad_desc* d) { return ssg_wgrad_bf16_ws_bytes(d, 1); }
extern "C" int ssg_conv2d_wgrad_bf16x1_f32(const ssg_wgrad_desc* d, void* stream) { return run<1>(d, stream); }

extern "C" int ssg_conv2d_wgrad_bf16x2_ok(const ssg_wgrad_desc* d) { return ssg_wgrad_bf16_shape_ok(d, 1) ? 1 : 0; }
extern "C" int ssg_conv2d_wgrad_bf16x2_kernel_id(const ssg_wgrad_desc* d) { return ssg_wgrad_bf16_shape_ok(d, 1) ? 92 : SSG_EINVAL; }
extern "C" int64_t ssg_conv2d_wgrad_bf16x2_workspace_bytes(const ssg_wgrad_desc* d) { return ssg_wgrad_bf16_ws_bytes(d, 1); }
extern "C" int ssg_conv2d_wgrad_bf16x2_f32(const ssg_wgrad_desc* d, void* stream) { return run<2>(d, stream); }
