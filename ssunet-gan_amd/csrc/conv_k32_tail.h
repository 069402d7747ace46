// Tail of the bf16 conv kernels on 16x16x32 MFMAs with 32-pixel tile rows (conv_halo_k32_bf16.hip, conv_s2_k32_x1.hip): the
// non-finite recompute and the epilogue from 16x16 accumulator fragments.  C/D map of a 16x16 MFMA as these kernels feed it
// (A = weights, B = pixels): acc[i][j][r] is grid pixel p = wm * WTM + i * 16 + l15 of the workgroup's TH x 32 tile, i.e.
// (ty * TH + (p >> 5), tx * 32 + (p & 31)), and output channel n0 + wn * WTN + j * 16 + kg * 4 + r, with l15 = lane & 15,
// kg = lane >> 4.
#pragma once
#include "common.h"
#include "conv_args.h"
#include "conv_slow.h"

// Non-finite operands (conv_slow.h): a workgroup that holds a non-finite accumulator recomputes its tile with fp32 FMAs over
// taps [0, NTAPS), one accumulator row group at a time so that the scratch (NI * 4 values per thread of the NT) fits the LDS
// allocation the caller asserts.  Called by every thread, after the main loop's last LDS read (the vote is a barrier).
template <int NTAPS, int TH, int WTM, int WTN, int NT, int MI, int NI>
__device__ __forceinline__ void ssg_k32_recompute_nonfinite(f32x4 (&acc)[MI][NI], unsigned char* lds, int tid, int n, int ty, int tx,
                                                            int n0, int wm, int wn, int kg, int l15) {
  constexpr int TW = 32;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) bad |= ssg_nonfinite(acc[i][j][r]);
  if (ssg_any_nonfinite(bad)) {
    float* scr = (float*)lds + tid;                      // value e of this thread at scr[e * NT]; only this thread reads it back
    const ConvArgs& as = *ssg_reload_args<ConvArgs>();
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int p = wm * WTM + i * 16 + l15;
#pragma unroll 1
      for (int e = 0; e < NI * 4; ++e) {
        const int co = n0 + wn * WTN + (e >> 2) * 16 + kg * 4 + (e & 3);
        scr[e * NT] = ssg_conv_slow_value<false>(as, n, ty * TH + (p >> 5), tx * TW + (p & 31), co, 0, NTAPS);
      }
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = scr[(j * 4 + r) * NT];
    }
  }
}

// Epilogue: bias, optional residual, ReLU / LeakyReLU, f32x4 stores.  Grid pixel (gy, gx) is output pixel (gy * out_sy + out_oy,
// gx * out_sx + out_ox); a.res may be null.  Cout % (WTN * waves) == 0 in every caller: every column is real.
// `a` BY VALUE: its fields are then scalars of the kernel, and the tests of a.res / a.act are hoisted out of the store loop as they
// were when this text stood in the kernels; through a reference the compiler re-tests them at every store (measured: 3 % on the
// one-term 64-channel 512^2 forward, whose time is mostly these stores).
template <int TH, int WTM, int WTN, int MI, int NI>
__device__ __forceinline__ void ssg_k32_epilogue(const ConvArgs a, const f32x4 (&acc)[MI][NI], int n, int ty, int tx, int n0, int wm,
                                                 int wn, int kg, int l15) {
  constexpr int TW = 32;
  size_t opix[MI]; bool pok[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int p = wm * WTM + i * 16 + l15;
    const int gy = ty * TH + (p >> 5), gx = tx * TW + (p & 31);
    pok[i] = gy < a.GH && gx < a.GW;
    opix[i] = (size_t)(n * a.OH + gy * a.out_sy + a.out_oy) * a.OW + gx * a.out_sx + a.out_ox;
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int co = n0 + wn * WTN + j * 16 + kg * 4;
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
