// Host side of the opt-in bf16 k32 family (internal, host code only): what conv_halo_k32_bf16.hip, conv_s2_k32_x1.hip,
// conv_wgrad_k32_bf16.hip and conv_wgrad_s2_k32_x1.hip share besides their kernels -- the descriptor checks, the argument blocks, the
// slab plan and the launch sequence.  A file keeps its kernels and the choice of the kernel to launch.
#pragma once
#include "conv_args.h"
#include "conv_wgrad_args.h"

// Column tile of a launch: 128 output channels per workgroup where Cout % 128 == 0, else 64.  Pack format code: 1000 * terms + tile.
inline int ssg_k32_bf16_bn(int Cout) { return Cout % 128 == 0 ? 128 : 64; }

// ---------------------------------------------------------------------------------------------------------------- convolution
// The three forms: the unit-stride 3x3 conv (one or two terms), the stride-2 3x3 forward, one parity class of its input gradient
enum K32Bf16Form { K32_UNIT, K32_S2_FWD, K32_S2_CLS };

// The descriptor as the kernel's argument block (a.w still the fp32 weights); false (with the reason in ssg_last_error when `why`)
// where the kernels do not take it.  `fam` names the family in the messages, `terms` sets the bytes per weight of the pack (2 * terms).
inline bool ssg_k32_bf16_conv_args(const ssg_conv_desc* d, ConvArgs& a, K32Bf16Form form, const char* fam, int terms, bool why) {
#define K32_NEED(cond, fmt, ...) do { if (!(cond)) { if (why) ssg_set_error("conv %s: " fmt, fam, ##__VA_ARGS__); return false; } } while (0)
  K32_NEED(d != nullptr, "null desc");
  K32_NEED(d->in1 && d->w && d->out, "null pointer");
  K32_NEED(!d->bnpart && !d->ws && !d->parity_merge && !d->in_scale && !d->in_shift && !d->bwd_x, "bnpart / ws / parity_merge / in_scale / bwd_x are not taken");
  K32_NEED(d->kmode == 0, "kmode 0 only");
  // ---- per form: taps, strides and offsets; the stride-2 forms take one input and no residual
  if (form == K32_UNIT) {
    K32_NEED(d->ntaps == 9 && d->in_sy == 1 && d->in_sx == 1 && d->out_sy == 1 && d->out_sx == 1 && d->out_oy == 0 && d->out_ox == 0,
             "the 9 taps of a unit-stride forward conv only");
    for (int t = 0; t < 9; ++t) K32_NEED(d->dy[t] >= -1 && d->dy[t] <= 1 && d->dx[t] >= -1 && d->dx[t] <= 1, "tap offset outside the 3x3 window");
  } else {
    K32_NEED(d->C2 == 0 && !d->in2 && !d->res, "one input and no residual");
    if (form == K32_S2_FWD) {
      K32_NEED(d->ntaps == 9 && d->in_sy == 2 && d->in_sx == 2 && d->out_sy == 1 && d->out_sx == 1 && d->out_oy == 0 && d->out_ox == 0,
               "the 9 taps of a stride-2 forward conv only");
      for (int t = 0; t < 9; ++t) K32_NEED(d->dy[t] == t / 3 - 1 && d->dx[t] == t % 3 - 1, "the taps are not the nine row-major taps of a 3x3 pad-1 window");
    } else {
      K32_NEED((d->ntaps == 1 || d->ntaps == 2 || d->ntaps == 4) && d->in_sy == 1 && d->in_sx == 1 && d->out_sy == 2 && d->out_sx == 2 &&
               (d->out_oy == 0 || d->out_oy == 1) && (d->out_ox == 0 || d->out_ox == 1),
               "1 / 2 / 4 taps at unit input stride, output stride 2 and offset 0 / 1 only");
      for (int t = 0; t < d->ntaps; ++t) K32_NEED((d->dy[t] == 0 || d->dy[t] == 1) && (d->dx[t] == 0 || d->dx[t] == 1), "tap offset outside {0, +1}");
    }
  }
  for (int t = 0; t < d->ntaps; ++t)                     // nine distinct taps inside the 3x3 window are the window
    for (int u = 0; u < t; ++u) K32_NEED(d->dy[t] != d->dy[u] || d->dx[t] != d->dx[u], "a tap twice");
  // ---- every form
  K32_NEED(d->C1 > 0 && d->C1 % 32 == 0 && d->C2 >= 0 && d->C2 % 32 == 0 && (d->C2 == 0 || d->in2), "C1=%d C2=%d must be multiples of 32", d->C1, d->C2);
  K32_NEED(d->Cout > 0 && d->Cout % 64 == 0, "Cout=%d must be a multiple of 64", d->Cout);
  K32_NEED(d->Kp == (d->C1 + d->C2) * d->ntaps, "Kp=%d != Cin*ntaps", d->Kp);
  K32_NEED(d->N > 0 && d->H > 0 && d->W > 0 && d->GH > 0 && d->GW >= 17, "empty grid or GW=%d < 17", d->GW);
  K32_NEED((long long)(d->GH - 1) * d->out_sy + d->out_oy < d->OH && (long long)(d->GW - 1) * d->out_sx + d->out_ox < d->OW, "pixel grid exceeds the output image");
  K32_NEED(d->ld1 >= d->C1 && d->ld1 % 4 == 0 && (d->C2 == 0 || (d->ld2 >= d->C2 && d->ld2 % 4 == 0)) && d->ldo >= d->Cout && d->ldo % 4 == 0 &&
           (!d->res || (d->ldr >= d->Cout && d->ldr % 4 == 0)), "pixel strides");
  K32_NEED(ssg_aligned16(d->in1) && (d->C2 == 0 || ssg_aligned16(d->in2)) && ssg_aligned16(d->w) && ssg_aligned16(d->out) && ssg_aligned16(d->res) && ssg_aligned16(d->bias),
           "16-B alignment");
  K32_NEED(d->act == SSG_ACT_NONE || d->act == SSG_ACT_RELU || d->act == SSG_ACT_LRELU, "act=%d", d->act);
  const int ld = form == K32_UNIT && d->ld2 > d->ld1 ? d->ld2 : d->ld1;      // the unit-stride form counts ld2 with or without a second input
  K32_NEED((unsigned long long)d->N * d->H * d->W * (unsigned long long)ld * 4ull <= 0xfffffff0ull, "input beyond the 32-bit byte offsets of the buffer descriptors");
  K32_NEED((unsigned long long)d->Cout * d->Kp * (2ull * terms) <= 0x7ffffff0ull, "weight pack beyond the 32-bit byte offsets");
#undef K32_NEED
  a = ssg_conv_to_args(d);
  return true;
}

// _ok: the pack format code the launch for `d` reads, or 0 where the launch refuses `d`
inline int ssg_k32_bf16_conv_fmt(const ssg_conv_desc* d, K32Bf16Form form, const char* fam, int terms) {
  ConvArgs a;
  return ssg_k32_bf16_conv_args(d, a, form, fam, terms, false) ? 1000 * terms + ssg_k32_bf16_bn(a.Cout) : 0;
}

// _f32: check, put the pack in a.w, launch.  `launch(a, stream)` chooses the kernel.
template <class Launch>
int ssg_k32_bf16_conv_run(const ssg_conv_desc* d, const void* pack, K32Bf16Form form, const char* fam, int terms, void* stream, Launch&& launch) {
  ConvArgs a;
  if (!ssg_k32_bf16_conv_args(d, a, form, fam, terms, true)) return SSG_EINVAL;
  SSG_REQUIRE(pack != nullptr, SSG_EINVAL, "conv %s: null weight pack", fam);
  SSG_REQUIRE(ssg_aligned16(pack), SSG_EALIGN, "conv %s: weight pack alignment", fam);
  a.w = (const float*)pack;                              // a.w32 keeps the fp32 weights for the slow path
  return launch(a, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------------ weight gradient
// One geometry for both strides and both term counts: a K-step is WG_BF16_KP pixels of one row of the dy grid, a tile 9 taps x
// WG_BF16_CB input channels x 32 * nj output channels, a slab WG_BF16_MIN_ROWS .. WG_BF16_MAX_ROWS K-steps (4096 pixels: wgrad_k32's).
constexpr int WG_BF16_KP = 32, WG_BF16_CB = 64, WG_BF16_MIN_ROWS = 8, WG_BF16_MAX_ROWS = 128;

// The shape test alone (no pointers), what the _ok entry points answer: the nine row-major taps of the 3x3 pad-1 window at input
// stride `stride` (1 or 2) over the whole image, 64-channel multiples, GW >= 17, tensors within 32-bit byte offsets, no in_scale.
// Stride 2 takes one input.
inline bool ssg_wgrad_bf16_shape_ok(const ssg_wgrad_desc* d, int stride) {
  if (!d || d->in_scale || d->in_shift) return false;
  if (d->ntaps != 9 || d->KH != 3 || d->KW != 3 || d->in_sy != stride || d->in_sx != stride) return false;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->GH != (d->H + stride - 1) / stride || d->GW != (d->W + stride - 1) / stride) return false;
  for (int t = 0; t < 9; ++t)
    if (d->dy[t] != t / 3 - 1 || d->dx[t] != t % 3 - 1 || d->ky[t] != t / 3 || d->kx[t] != t % 3) return false;
  if (d->C1 <= 0 || d->C1 % 64 || d->C2 < 0 || d->C2 % 64 || (stride == 2 && d->C2) || d->Cout <= 0 || d->Cout % 64 || d->GW < 17) return false;
  if (d->Cin_real != d->C1 + d->C2) return false;
  if ((d->ld1 & 3) || d->ld1 < d->C1 || (d->C2 && ((d->ld2 & 3) || d->ld2 < d->C2)) || (d->ldd & 3) || d->ldd < d->Cout) return false;
  const int ld = stride == 1 && d->ld2 > d->ld1 ? d->ld2 : d->ld1;           // unit stride counts ld2 with or without a second input
  const unsigned long long xb = (unsigned long long)d->N * d->H * d->W * (unsigned long long)ld * 4ull;
  const unsigned long long db = (unsigned long long)d->N * d->GH * d->GW * (unsigned long long)d->ldd * 4ull;
  return xb <= 0xfffffff0ull && db <= 0xfffffff0ull;
}

struct WgBf16Plan { int nj, mt, nt, splits, steps_per_split; int64_t ws_bytes; };

// Tiles, slabs (ssg_wgrad_slabs) and the bytes of the slabs [split][9 * Cin][Cout] of a shape that passed ssg_wgrad_bf16_shape_ok: a
// function of the shape alone
inline WgBf16Plan ssg_wgrad_bf16_plan(const ssg_wgrad_desc* d) {
  WgBf16Plan p;
  p.nj = ssg_k32_bf16_bn(d->Cout) / 32;
  p.mt = (d->C1 + d->C2) / WG_BF16_CB; p.nt = d->Cout / (32 * p.nj);
  const long long steps = (long long)d->N * ((d->GW + WG_BF16_KP - 1) / WG_BF16_KP) * d->GH;
  const WgSlabs s = ssg_wgrad_slabs(steps, (long long)p.mt * p.nt, WG_BF16_MIN_ROWS, WG_BF16_MAX_ROWS);
  p.splits = s.splits; p.steps_per_split = s.steps_per_split;
  p.ws_bytes = (int64_t)p.splits * 9 * (d->C1 + d->C2) * d->Cout * (int64_t)sizeof(float);
  return p;
}

// _workspace_bytes: 0 where the shape is refused
inline int64_t ssg_wgrad_bf16_ws_bytes(const ssg_wgrad_desc* d, int stride) {
  return ssg_wgrad_bf16_shape_ok(d, stride) ? ssg_wgrad_bf16_plan(d).ws_bytes : 0;
}

// _f32: validate, launch the slabs, reduce them in order.  `fam`: the family's name in the messages; `launch(nj, a, grid, stream)`
// chooses the kernel.
template <class Launch>
int ssg_wgrad_bf16_run(const ssg_wgrad_desc* d, int stride, const char* fam, void* stream, Launch&& launch) {
  SSG_REQUIRE(d && d->in1 && d->dout && d->dw_oihw && d->ws, SSG_EINVAL, "wgrad %s: null pointer", fam);
  SSG_REQUIRE(d->C2 == 0 || d->in2, SSG_EINVAL, "wgrad %s: C2 > 0 needs in2", fam);
  SSG_REQUIRE(ssg_wgrad_bf16_shape_ok(d, stride), SSG_EINVAL,
              "wgrad %s: not the 3x3 stride-%d pad-1 weight gradient with C1 %% 64 == C2 %% 64 == Cout %% 64 == 0 (C2 == 0 at stride 2), GW >= 17, "
              "32-bit byte offsets and no in_scale (C1=%d C2=%d Cout=%d GW=%d ntaps=%d stride=%d)", fam, stride, d->C1, d->C2, d->Cout, d->GW, d->ntaps, d->in_sy);
  SSG_REQUIRE(ssg_aligned16(d->in1) && (stride == 2 || ssg_aligned16(d->in2)) && ssg_aligned16(d->dout) && ssg_aligned16(d->ws), SSG_EALIGN,
              "wgrad %s: alignment", fam);
  const WgBf16Plan p = ssg_wgrad_bf16_plan(d);
  SSG_REQUIRE(d->ws_bytes >= p.ws_bytes, SSG_EINVAL, "wgrad %s: workspace too small", fam);
  hipStream_t st = (hipStream_t)stream;
  const WgArgs a = ssg_wgrad_args(d, p.steps_per_split); // no in_scale (the shape test), xcd_swizzle 0
  const int rc = launch(p.nj, a, dim3((unsigned)p.mt, (unsigned)p.nt, (unsigned)p.splits), st);
  if (rc != SSG_OK) return rc;
  return ssg_wgrad_reduce_launch(d, p.splits, st);
}
