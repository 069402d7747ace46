// Split-operand (bf16x3) weight gradient of the LDS-DMA family, split-once body on v_mfma_f32_16x16x32_bf16.  Same WgArgs, grid
// semantics (row block of 128 (tap, ci) rows, column block of BN output channels, K-slice bz, XCD remap), K-slices
// (pixels [bz * steps_per_split * 16, ...) of the flat N x GH x GW range, clipped to Ptot) and slab layout as wgrad_dma_x3_kernel
// (conv_wgrad_dma.hip), which it replaces wherever ssg_wgrad_dma_k32_ok holds.  What differs, after conv_wgrad_k32.hip:
//   * every fp32 element is loaded and split ONCE per workgroup, on the way from HBM into LDS (buffer loads -> registers -> split3_4
//     -> three bf16 planes [pixel][64 rows], 128-byte rows per 64-row half, conv_wgrad_k32.hip's chunk XOR), where the old body
//     splits every fragment in each of the two waves that consume it (~180 VALU per wave and 24 MFMAs);
//   * fragments leave LDS by ds_read_b64_tr_b16, two per 16x16x32 operand; 2 x 2 waves of 64 x 64 (BN = 64: 64 x 32);
//   * a K-step = 32 pixels of the flat range: 96 (48) MFMAs per wave between the barriers.  A slice is a whole number of 16-pixel
//     units, so its last step may be half empty: pixels at or beyond the slice's end are loaded as zeros on both operands
//     (out-of-range buffer offsets), as are out-of-image taps, rows >= M and columns >= Cout;
//   * planes are single-buffered (48 KB at BN = 128, 36 KB at BN = 64: two workgroups per CU), the next step's loads are in flight in
//     registers across the MFMAs.
// CAT: the row block may hold channels of both inputs of a concat; a buffer load takes ONE (scalar) resource, so every A piece is
// loaded from both with the other's lanes out of range (they return zeros and move no data) and the two are ORed.
#include "common.h"
#include "lds_dma.h"
#include "conv_wgrad_args.h"
#include "mfma_split.h"
#include "conv_slow.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int KP = 32;                     // pixels per K-step
constexpr int BM = 128;
constexpr int PLANE = KP * 128;            // one bf16 plane of one 64-row half: [32 pixels][64 rows]
constexpr int HALF = 3 * PLANE;
constexpr int AIMG = 2 * HALF;

// 16-byte chunk c (0..7) of pixel row p sits at chunk position c ^ sw(p) (conv_wgrad_k32.hip)
__device__ __forceinline__ int sw(int p) { return ((((p >> 1) & 1) | (((p >> 3) & 1) << 1)) << 1); }

template <int BN, bool CAT>
__global__ __launch_bounds__(256, 2) void wgrad_dma_x3_k32_kernel(const WgArgs a) {
  constexpr int NH = BN / 64;              // 64-column halves of the dy image
  constexpr int PXS = 1024 / BN;           // pixels one pass of the 256 threads stages: 8 / 16
  constexpr int B_PC = KP / PXS;           // dy pieces per thread and step: 4 / 2
  constexpr int A_PC = 4;                  // x pieces per thread and step: pixels s_px + 8j of one row quad
  constexpr int NI = BN / 32;              // 16-column fragments per wave: 4 / 2
  __shared__ __attribute__((aligned(1024))) unsigned char lds[AIMG + NH * HALF];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, g = lane >> 4;
  // workgroup -> (row block, column block, K slice): wgrad_dma_body's map (sharers of an operand on one XCD)
  int bx = blockIdx.x, grp = blockIdx.y + gridDim.y * blockIdx.z;
  if (a.xcd_swizzle) {
    const int mt = gridDim.x, G = gridDim.y * gridDim.z;
    const int L = bx + mt * grp;
    if (L < (G >> 3) * 8 * mt) {
      const int q = L >> 3;
      bx = q % mt; grp = (q / mt) * 8 + (L & 7);
    }
  }
  const int by = grp % (int)gridDim.y, bz = grp / (int)gridDim.y;
  const int m0 = bx * BM, n0 = by * BN;
  const int Cin = a.C1 + a.C2;

  // ---- this workgroup's pixels [P0, P1) (32-bit: ssg_wgrad_dma_k32_ok)
  const long long P0l = (long long)bz * a.steps_per_split * 16;
  long long P1l = P0l + (long long)a.steps_per_split * 16;
  if (P1l > a.Ptot) P1l = a.Ptot;
  const int P0 = (int)(P0l < a.Ptot ? P0l : a.Ptot), P1 = (int)(P1l > P0l ? P1l : P0);
  const int nsteps = (P1 - P0 + KP - 1) / KP;

  const unsigned OOB = 0xffffffffu;
  const unsigned npix_in = (unsigned)a.N * (unsigned)a.H * (unsigned)a.W;
  const auto x1_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in1), 0, (int)(((npix_in - 1u) * (unsigned)a.ld1 + (unsigned)a.C1) * 4u), 0x00020000);
  const auto x2_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in2), 0, (int)(((npix_in - 1u) * (unsigned)a.ld2 + (unsigned)(CAT ? a.C2 : a.C1)) * 4u), 0x00020000);
  const auto d_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dout), 0, (int)((((unsigned)a.Ptot - 1u) * (unsigned)a.ldd + (unsigned)((a.Cout + 3) & ~3)) * 4u), 0x00020000);

  // ---- x pieces: this thread's row quad (one tap, four channels of one input) at pixels s_px + 8j of the step
  const int a_rq = tid & 31, a_px = tid >> 5;
  const int a_row = m0 + 4 * a_rq;
  const bool a_rowok = a_row < a.M;
  int a_t = 0, a_c = 0;
  if (a_rowok) { a_t = a_row / Cin; a_c = a_row - a_t * Cin; }
  const int a_dy = ssg_tap_dy(a.tap_bits, a_t), a_dx = ssg_tap_dx(a.tap_bits, a_t);
  const bool a_first = !CAT || a_c < a.C1;
  const unsigned a_ldb = (unsigned)(a_first ? a.ld1 : a.ld2) * 4u;
  const unsigned a_cho = (unsigned)(a_first ? a_c : a_c - a.C1) * 4u;
  int a_nH[A_PC], a_gy[A_PC], a_gx[A_PC];                // running coordinate of piece j's pixel (n * H, gy, gx)
  {
    const int GHW = a.GH * a.GW;
#pragma unroll
    for (int j = 0; j < A_PC; ++j) {
      const int P = P0 + a_px + 8 * j;
      const int n = P / GHW, rem = P - n * GHW;
      a_gy[j] = rem / a.GW; a_gx[j] = rem - a_gy[j] * a.GW; a_nH[j] = n * a.H;
    }
  }
  int a_P = P0 + a_px;                                   // flat index of piece 0's pixel
  const int a_dst = (a_rq >> 4) * HALF + a_px * 128 + (((((a_rq & 15) >> 1)) ^ sw(a_px)) << 4) + (a_rq & 1) * 8;

  // ---- dy pieces: column quad b_cq at pixels b_px + PXS * j
  const int b_cq = tid & (BN / 4 - 1), b_px = tid / (BN / 4);
  const bool b_colok = n0 + 4 * b_cq < a.Cout;
  int b_P = P0 + b_px;
  unsigned b_off = ((unsigned)b_P * (unsigned)a.ldd + (unsigned)(n0 + 4 * b_cq)) * 4u;
  const unsigned b_step = (unsigned)a.ldd * 4u;
  const int b_dst = AIMG + (b_cq >> 4) * HALF + b_px * 128 + (((((b_cq & 15) >> 1)) ^ sw(b_px)) << 4) + (b_cq & 1) * 8;

  struct Raw { u32x4 x[A_PC]; u32x4 x2[CAT ? A_PC : 1]; u32x4 d[B_PC]; };
  auto load = [&](Raw& r) {                              // the step at (a_P, b_P); advances both by one step
#pragma unroll
    for (int j = 0; j < A_PC; ++j) {
      const int iy = a_gy[j] * a.in_sy + a_dy, ix = a_gx[j] * a.in_sx + a_dx;
      const bool ok = a_rowok && a_P + 8 * j < P1 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      const unsigned off = (unsigned)((a_nH[j] + iy) * a.W + ix) * a_ldb + a_cho;
      r.x[j] = __builtin_amdgcn_raw_buffer_load_b128(x1_rs, (ok && a_first) ? off : OOB, 0, 0);
      if constexpr (CAT) r.x2[j] = __builtin_amdgcn_raw_buffer_load_b128(x2_rs, (ok && !a_first) ? off : OOB, 0, 0);
      a_gx[j] += KP;
      while (a_gx[j] >= a.GW) { a_gx[j] -= a.GW; if (++a_gy[j] >= a.GH) { a_gy[j] = 0; a_nH[j] += a.H; } }
    }
    a_P += KP;
#pragma unroll
    for (int j = 0; j < B_PC; ++j) {
      const bool ok = b_colok && b_P + PXS * j < P1;
      r.d[j] = __builtin_amdgcn_raw_buffer_load_b128(d_rs, ok ? b_off + (unsigned)(PXS * j) * b_step : OOB, 0, 0);
    }
    b_P += KP; b_off += (unsigned)KP * b_step;
  };
  auto put = [&](unsigned char* base, u32x4 raw) {
    bf16x4 p1, p2, p3;
    split3_4(__builtin_bit_cast(f32x4, raw), p1, p2, p3);
    *(bf16x4*)base = p1; *(bf16x4*)(base + PLANE) = p2; *(bf16x4*)(base + 2 * PLANE) = p3;
  };
  auto store = [&](const Raw& r) {
    // pixel + 8j: sw() changes with pixel bit 3 (chunk ^ 4 = byte ^ 64); + 16j: unchanged
#pragma unroll
    for (int j = 0; j < A_PC; ++j) {
      u32x4 v = r.x[j];
      if constexpr (CAT) v |= r.x2[j];
      put(lds + (a_dst ^ ((j & 1) << 6)) + j * 8 * 128, v);
    }
#pragma unroll
    for (int j = 0; j < B_PC; ++j)
      put(lds + (PXS == 8 ? (b_dst ^ ((j & 1) << 6)) : b_dst) + j * PXS * 128, r.d[j]);
  };

  // ---- transposed-read addresses (conv_wgrad_k32.hip): operand k-group g covers pixels 8g .. 8g + 7 of the step; lane 4q + pp of the
  // group supplies pixel row q (the second read adds 4: + 512 bytes, same sw), rows 4pp .. 4pp + 3 of the 16-row block blk
  const int q4 = l15 >> 2, pp = l15 & 3;
  int aoff[4], boff[NI];
  {
    const int p = 8 * g + q4;
    auto off = [&](int blk) { return p * 128 + (((2 * blk + (pp >> 1)) ^ sw(p)) << 4) + (pp & 1) * 8; };
#pragma unroll
    for (int i = 0; i < 4; ++i) aoff[i] = off(i);
#pragma unroll
    for (int j = 0; j < NI; ++j) boff[j] = off(NH == 2 ? j : 2 * wn + j);
  }
  auto frag = [&](const unsigned char* base, int o) -> bf16x8 {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + o));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + o + 512));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
  };
  const unsigned char* const Ab = lds + wm * HALF;
  const unsigned char* const Bb = lds + AIMG + (NH == 2 ? wn * HALF : 0);

  f32x4 acc[4][NI];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nsteps > 0) { Raw r; load(r); store(r); }
  for (int s = 0; s < nsteps; ++s) {
    wait_lds_reads();
    __builtin_amdgcn_s_barrier();                        // the step's planes are written
    asm volatile("" ::: "memory");
    const bool more = s + 1 < nsteps;
    Raw nx;
    if (more) load(nx);

    bf16x8 df[NI][3];
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) df[j][q] = frag(Bb + q * PLANE, boff[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x8 xf[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) xf[q] = frag(Ab + q * PLANE, aoff[i]);
      // small terms first; A = dy (rows = output channels), B = x (columns = (tap, ci) rows of the slab)
#define SSG_WD_TERM(QD, QX)                                                                       \
  _Pragma("unroll") for (int j = 0; j < NI; ++j)                                                  \
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[j][QD], xf[QX], acc[i][j], 0, 0, 0);
      SSG_WD_TERM(2, 0) SSG_WD_TERM(1, 1) SSG_WD_TERM(0, 2)
      SSG_WD_TERM(1, 0) SSG_WD_TERM(0, 1)
      SSG_WD_TERM(0, 0)
#undef SSG_WD_TERM
    }
    if (more) {
      wait_lds_reads();
      __builtin_amdgcn_s_barrier();                      // every wave has read this step's planes
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      store(nx);
    }
  }

  // acc[i][j][r] = (row m0 + wm * 64 + i * 16 + l15, column n0 + wn * (BN / 2) + j * 16 + 4g + r)
  const int row0 = m0 + wm * 64 + l15, co0 = n0 + wn * (BN / 2) + 4 * g;
  wait_lds_reads();
  {                                                      // non-finite operands: conv_slow.h
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) bad |= ssg_nonfinite(acc[i][j][r]);
    if (ssg_any_nonfinite(bad)) {
      const WgArgs& as = *ssg_reload_args<WgArgs>();
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          ssg_slow_refill4(acc[i][j], (float*)lds + tid, 256, [&](int r) {
            const int row = row0 + i * 16;
            const int t = row / Cin;
            return ssg_wgrad_slow_value_flat(as, t, row - t * Cin, co0 + j * 16 + r, (long long)P0, (long long)P1);
          });
    }
  }
  float* slab = a.ws + (size_t)bz * a.M * a.Cout;
  const bool vec = (a.Cout & 3) == 0;                    // then the slab rows are 16-byte aligned (M % 4 == 0)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + i * 16;
    if (row >= a.M) continue;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int co = co0 + j * 16;
      float* p = slab + (size_t)row * a.Cout + co;
      if (vec) {
        if (co < a.Cout) *(f32x4*)p = acc[i][j];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (co + r < a.Cout) p[r] = acc[i][j][r];
      }
    }
  }
}

}  // namespace

// The split-once body serves a launch whose channel counts and row strides are whole quads, whose tensors are 16-byte aligned
// (one buffer load = one quad) and lie within 32-bit byte offsets (buffer offsets are 32 bits; the pixel index then fits an int).
bool ssg_wgrad_dma_k32_ok(const WgArgs& a) {
  if ((a.C1 & 3) || (a.C2 & 3) || (a.ld1 & 3) || (a.ld2 & 3) || (a.ldd & 3)) return false;
  if (!ssg_aligned16(a.in1) || !ssg_aligned16(a.in2) || !ssg_aligned16(a.dout) || !ssg_aligned16(a.ws)) return false;
  if (a.N < 1 || a.H < 1 || a.W < 1 || a.GH < 1 || a.GW < 1 || a.Ptot < 1) return false;
  const unsigned long long npix = (unsigned long long)a.N * a.H * a.W;
  const unsigned long long ld = (unsigned long long)(a.ld1 > a.ld2 ? a.ld1 : a.ld2);
  if (npix * ld * 4ull > 0xfffffff0ull) return false;
  if (((unsigned long long)a.Ptot + 16ull * (unsigned long long)a.steps_per_split + 64ull) * (unsigned long long)a.ldd * 4ull > 0xfffffff0ull) return false;
  return true;
}

int ssg_wgrad_dma_k32_launch(const WgArgs& a, int variant, dim3 grid, hipStream_t st) {
  if (variant == 0) {
    if (a.C2) hipLaunchKernelGGL((wgrad_dma_x3_k32_kernel<128, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((wgrad_dma_x3_k32_kernel<128, false>), grid, dim3(256), 0, st, a);
  } else {
    if (a.C2) hipLaunchKernelGGL((wgrad_dma_x3_k32_kernel<64, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((wgrad_dma_x3_k32_kernel<64, false>), grid, dim3(256), 0, st, a);
  }
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}
