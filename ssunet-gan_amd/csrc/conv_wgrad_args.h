// Kernel-argument block shared by the two weight-gradient kernels (internal).
#pragma once
#include "common.h"

struct WgArgs {
  const float* in1; const float* in2; const float* dout; float* ws;
  int C1, C2, ld1, ld2, N, H, W, Cout, ldd, GH, GW, in_sy, in_sx, ntaps;
  unsigned long long tap_bits;
  int M;                 // ntaps * Cin
  long long Ptot;        // N*GH*GW
  int steps_per_split;   // K-steps (16 pixels each) per z-slice
  int xcd_swizzle;       // conv_wgrad_dma.hip: sharers of an operand on one XCD (set by the launcher)
  const float* in_scale; const float* in_shift; int in_act; float in_slope;   // ssg_wgrad_desc.in_scale (conv_wgrad_k32.hip)
};


// conv_wgrad_dma.hip: LDS-DMA pipeline for Cout > 32 (variant 0 = <128,128>, 1 = <128,64>)
int ssg_wgrad_dma_launch(const WgArgs& a, int variant, dim3 grid, hipStream_t st, bool split);
// which body a split launch runs: 1 = wgrad_dma_x3_kernel (operands split as they leave LDS), 2 = the split-once body below
int ssg_wgrad_dma_split_body(const WgArgs& a, int variant, long long workgroups);

// conv_wgrad_dma_k32.hip: the split (bf16x3) form of the above with operands split once on the way into LDS, 32-pixel K-steps on
// v_mfma_f32_16x16x32_bf16; same grid, K-slices and slabs.  Chosen inside ssg_wgrad_dma_launch where ssg_wgrad_dma_k32_ok holds.
bool ssg_wgrad_dma_k32_ok(const WgArgs& a);
int ssg_wgrad_dma_k32_launch(const WgArgs& a, int variant, dim3 grid, hipStream_t st);

// conv_wgrad_halo.hip: 3x3 stride-1 weight gradient with an LDS-resident pixel window
// (variant 0 = 9 taps x 32 channels x 128 output channels per workgroup, 1 = 9 x 64 x 64)
int ssg_wgrad_halo_cb(int variant);
bool ssg_wgrad_halo_ok(const ssg_wgrad_desc* d, int variant);
int ssg_wgrad_halo_launch(const WgArgs& a, int variant, dim3 grid, hipStream_t st, bool split);   // split: operands as three bf16 terms on the bf16 pipe

// conv_wgrad_k32.hip (round 4): split operands on v_mfma_f32_16x16x32_bf16, 9 x 64 x 64 tiles of 512 threads, rolling 3-row window
bool ssg_wgrad_k32_ok(const ssg_wgrad_desc* d);
long long ssg_wgrad_k32_steps(const ssg_wgrad_desc* d);
int ssg_wgrad_k32_launch(const WgArgs& a, dim3 grid, hipStream_t st);

// conv_wgrad.hip: the kernels' argument block of a validated descriptor, and the ordered slab reduce (wgrad_reduce_kernel), also for
// the bf16 launchers (conv_k32_bf16_host.h), which plan and launch on their own
WgArgs ssg_wgrad_args(const ssg_wgrad_desc* d, int steps_per_split);
int ssg_wgrad_reduce_launch(const ssg_wgrad_desc* d, int splits, hipStream_t st);

// Slab count of the kernels whose K-step is one image row of a 32-pixel column strip (wgrad_k32 and the bf16 family).  A slab is one
// workgroup's accumulation chain of min_rows .. max_rows K-steps; within that, the count that leaves the fewest CUs idle in the last
// wave of 256 workgroups (one workgroup per CU): the first best of at most 1025 counts, the scan ending early at 97 % of a full wave.
struct WgSlabs { int splits, steps_per_split; };
inline WgSlabs ssg_wgrad_slabs(long long steps, long long tiles, long long min_rows, long long max_rows) {
  const long long lo = (steps + max_rows - 1) / max_rows;
  long long hi = steps / min_rows;
  if (hi < lo) hi = lo;
  long long best = lo; double beff = 0;
  for (long long sp = lo; sp <= hi && sp <= lo + 1024; ++sp) {
    const long long wg = sp * tiles;
    const double eff = (double)wg / (256.0 * ((wg + 255) / 256));
    if (eff > beff + 1e-9) { beff = eff; best = sp; }
    if (eff >= 0.97 && wg >= 256) break;
  }
  WgSlabs s;
  s.steps_per_split = (int)((steps + best - 1) / best);
  s.splits = (int)((steps + s.steps_per_split - 1) / s.steps_per_split);
  return s;
}
