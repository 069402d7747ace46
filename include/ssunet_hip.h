/* ssunet_hip.h -- C-ABI of the MI355X (gfx950) hot-path library for ssUnet-GAN training.
 *
 * The reference (ideafisher/ssUnet-GAN) is pure Python on stock PyTorch ops; it has no FFI
 * layer.  The drop-in boundary a maintainer sees is the Python nn.Module / train() surface
 * (the modules under ssunet-gan_amd/ mirror scripts/); THIS header is the build-defined C-ABI one
 * level below it: one entry point per stock torch op the reference's hot
 * path dispatches.  Each entry cites the reference call site(s) whose torch op it replaces
 * (paths relative to the reference's scripts/).
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless noted;
 *   - every call enqueues on `stream` (a hipStream_t passed as void*) and returns at once;
 *   - return value: 0 = ok, otherwise a negative SSG_E* code or a positive hipError_t;
 *     ssg_last_error() returns a thread-local message.  Nothing throws across the ABI;
 *   - the library allocates nothing and keeps no state between calls: callers own all
 *     buffers including workspaces (sizes via the *_workspace_bytes helpers);
 *   - activations are fp32 "NHWC with pixel stride": element (n,y,x,c) of a tensor with
 *     H x W pixels lives at ((n*H + y)*W + x)*ld + c, ld >= C, ld % 4 == 0, 16-B aligned.
 */
#ifndef SSUNET_HIP_H
#define SSUNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSG_OK 0
#define SSG_EINVAL (-1)   /* bad argument / unsupported shape */
#define SSG_EALIGN (-2)   /* pointer or stride alignment */

#define SSG_ACT_NONE 0
#define SSG_ACT_RELU 1
#define SSG_ACT_LRELU 2
#define SSG_ACT_SWISH 3   /* x*sigmoid(x) (efficientnet_pytorch/utils.py:37-48); batch-norm apply / backward only */

#define SSG_MAX_TAPS 9

const char* ssg_last_error(void);
int ssg_abi_version(void);

/* ------------------------------------------------------------------ convolution (MFMA)
 * Implicit-GEMM convolution, fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32.
 * Replaces F.conv2d forward and its input-gradient at: archs.py:210,212,218 (BasicBlock
 * 3x3 + 1x1 shortcut), archs.py:593-615 (1x1 heads, final), normalization.py:90-96 (SPADE
 * 3x3), models_seg_gan.py:37-39 (discriminator 3x3 s1/s2), models_seg_gan.py:281-283
 * (fc1/fc2 as 1x1 on a 1x1 grid).  torch.cat at archs.py:651-667 is absorbed by the
 * second input pointer.
 *
 * One launch computes, for every pixel (n,gy,gx) of a GH x GW grid and every co < Cout:
 *   acc = sum_t sum_c  in[n, gy*in_sy + dy[t], gx*in_sx + dx[t], c] * w[co, k(t,c)]
 * (out-of-image taps read 0), then  v = acc (+bias[co]) (+res[pixel,co]) -> act -> out at
 * pixel (gy*out_sy + out_oy, gx*out_sx + out_ox) of an OH x OW image.  `in` is the
 * channel-concatenation of in1 (C1 channels) and in2 (C2 channels, may be NULL/0).
 * Forward conv, stride-1 dgrad (taps mirrored) and stride-2 dgrad (4 parity launches)
 * are all instances of this.
 *
 * Weight operand `w` is a packed matrix [Cout][Kp] (row stride Kp floats, Kp % 16 == 0)
 * produced by ssg_pack_weights, whose K order must match `kmode`:
 *   kmode 0 (requires Cin % 16 == 0): k = (c/16)*ntaps*16 + t*16 + c%16
 *   kmode 1 (Cin % 4 == 0)          : k = t*Cin + c, zero padded to Kp
 */
typedef struct {
  const float* in1; const float* in2;
  int C1, C2, ld1, ld2;
  int N, H, W;              /* input image size */
  const float* w; int Kp; int kmode;
  const float* bias;        /* [Cout] or NULL */
  const float* res; int ldr;/* residual, indexed like out, or NULL */
  float* out; int Cout, ldo;
  int GH, GW;               /* pixel grid of this launch */
  int OH, OW;               /* output image size */
  int in_sy, in_sx, out_sy, out_sx, out_oy, out_ox;
  int ntaps; int dy[SSG_MAX_TAPS]; int dx[SSG_MAX_TAPS];   /* each in [-2, 5] */
  int act; float slope;
  double* bnpart;           /* optional batch-norm statistics of the OUTPUT (acc + bias, before res / act): one row [2][Cout]
                             * (sum, sum of squares; fp64) per M-tile, ssg_conv2d_bnpart_rows(d) rows; NULL = off */
  float* ws; int64_t ws_bytes;  /* optional split-K workspace (ssg_conv2d_workspace_bytes(d) bytes, 16-byte aligned); NULL = never split */
  const void* w_split;      /* optional: the same weights split into three bf16 terms by ssg_pack_weights_split_bf16x3 for the column
                             * tile ssg_conv2d_split_bn(d) reports; non-NULL selects the split-operand kernel (below).  NULL = fp32 MFMA */
  int parity_merge;         /* 1 = the launch is the whole input gradient of a 3x3 stride-2 pad-1 conv (models_seg_gan.py:37-39, s2 blocks):
                             * its 9 taps are the four output-parity classes in the order (0,0) | (0,1) x2 | (1,0) x2 | (1,1) x4, tap t of
                             * class (py, px) accumulates into output pixel (2 gy + py, 2 gx + px); GH x GW = ceil(OH/2) x ceil(OW/2),
                             * out_sy = out_sx = 2, out_oy = out_ox = 0, no bias / res / bnpart, w_split for a 64-column tile.  Only
                             * where ssg_conv2d_split_bn(d) returns 64 for such a descriptor; otherwise the caller launches the classes
                             * one by one (parity_merge = 0, ntaps = 1 / 2 / 2 / 4, out_oy / out_ox = the class).  0 = plain conv. */
  /* ABI 8: fused batch-norm apply on the INPUT (archs.py:229-230, relu(bn1(conv1(x))) feeding conv2): the launch convolves
   * act_in(in1[p][c] * in_scale[c] + in_shift[c]) -- the tensor ssg_bn_apply_f32 would have written, same fp32 fma, never
   * materialised; zero padding applies to the ACTIVATED tensor.  in_scale = NULL: off.  Only where ssg_conv2d_in_affine_ok(d)
   * returns 1 (split-operand k32 kernels, one input pointer, C1 <= 512, in_act none / ReLU / leaky ReLU). */
  const float* in_scale; const float* in_shift; int in_act; float in_slope;
  /* ABI 9: batch-norm BACKWARD statistics in the epilogue of the input-gradient launch that produces the gradient of an activation
   * y = act(x * scale[c] + shift[c]) (archs.py:229-230: the dgrad of conv2 produces d(relu(bn1(c1)))): the launch multiplies its result by
   * act'(.) recomputed from bwd_x (= c1, same shape and pixel order as `out`, pixel stride bwd_ldx) with bwd_scale / bwd_shift, WRITES THE
   * MASKED GRADIENT g, and fills `bnpart` (which must be set) with per-tile rows (sum g, sum g * (x - bwd_mean[c])) instead of the forward's
   * (sum, sum of squares): what ssg_bn_bwd_reduce_f32 would have read g and x again for.  bwd_x = NULL: off.  Only where
   * ssg_conv2d_bwd_stats_ok(d) returns 1 (the wide split-operand k32 tiles; no res, act, in_scale). */
  const float* bwd_x; int bwd_ldx; const float* bwd_scale; const float* bwd_shift; const float* bwd_mean; int bwd_act; float bwd_slope;
} ssg_conv_desc;

/* fp32 convolution on the bf16 matrix pipe (3x3, unit stride; archs.py:210,212 and their input gradients, models_seg_gan.py:37-39
 * stride-1 blocks): every fp32 operand is x = x1 + x2 + x3 with bf16 terms (24 significand bits, exact residuals) and the six
 * products of order >= 2^-16 go through v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- one fp32 ulp per product is left
 * out, results agree with the fp32-MFMA kernel to fp32 accumulation accuracy (tests/test_split_gpu.py), at 16/6 of its
 * matrix rate.  ssg_conv2d_split_bn: 0 when the launch for `d` has no split-operand kernel, else the column tile (64 / 128)
 * its weights must be split for: `w_split` = ssg_pack_weights_split_bf16x3(d->w rows [R][Kp] in kmode 0, R, Kp, BN) --
 * ssg_pack_weights_split_bytes bytes, layout [ceil(R/BN)][Kp/16][BN][96 B]: the 96 bytes of a row and 16-channel K-step are six
 * 16-byte slots, bf16 term p (0..2) of channels 8h .. 8h+7 of the step in slot (2p + h) ^ ((row >> 3) & 1); rows beyond R are zeros.
 * ABI 7 (round 4): ssg_conv2d_split_bn may also return 1128 or 1064 -- the launch goes to the 32-channel-chunk kernel on
 * v_mfma_f32_16x16x32_bf16 (conv_igemm_halo_k32.hip: 8 x 32-pixel x 128-channel tiles of 512 threads, or 4 x 32 x 64 of 256), whose
 * weights are packed by the same two functions with BN = that code: layout [R/bn][Kp/32 steps = chunk32 * 9 + tap][bn/16
 * fragments][3 planes][64 lanes][16 B] (bn = code - 1000; R % bn == 0, Kp % 288 == 0; lane l of fragment j holds bf16 term `plane` of row
 * j*16 + (l & 15), channels chunk32*32 + (l >> 4)*8 .. +7; 1016 / 1032, for Cout 12..16 / 17..32: R <= bn, one tile padded with zero
 * rows).  The value is always the pack format the
 * launch reads, whichever kernel reads it (the 16 x 32-pixel x 64-channel tiles of 512 threads read the pack of 1064;
 * ssg_conv2d_kernel_id tells the kernels apart).  ssg_conv_set_k32_mode(0 / 1 / 2): never /
 * where the grid fills the chip (default, SSG_K32) / wherever the shape is legal (tests). */
int ssg_conv2d_split_bn(const ssg_conv_desc* d);
int ssg_conv2d_in_affine_ok(const ssg_conv_desc* d);   /* ABI 8: 1 when the launch for `d` (w_split set) takes in_scale / in_shift */
int ssg_conv2d_bwd_stats_ok(const ssg_conv_desc* d);   /* ABI 9: 1 when the launch for `d` (w_split set) takes bwd_x ... */
int ssg_conv_set_k32_mode(int mode);
int64_t ssg_pack_weights_split_bytes(int R, int Kp, int BN);
int ssg_pack_weights_split_bf16x3(const float* w_packed, int R, int Kp, int BN, void* out, void* stream);

/* Opt-in bf16 INFERENCE convolution (conv_halo_k32_bf16.hip): the 3x3 stride-1 pad-1 forward conv of an eval-mode BasicBlock
 * (archs.py:210,212 under model.eval(), api.py:376-390) with both operands rounded ONCE to bf16 (round to nearest even) and one
 * v_mfma_f32_16x16x32_bf16 per product, fp32 accumulation, fp32 tensors in HBM.  An APPROXIMATION: |error| <= (2^-8 + 2^-18) *
 * conv(|x|, |w|) from the operand rounding, plus fp32 accumulation.  Never selected by ssg_conv2d_f32; no mode, no environment
 * variable: the caller launches it by name.  Non-finite results are those of the fp32 kernels (a tile that meets one is recomputed
 * in fp32: an fp32 value above ~3.39e38 rounds to bf16 infinity).
 * ssg_conv2d_bf16x1_ok: 0, or the pack format code (1128 / 1064 = 8 x 32-pixel x 128- / 64-channel tiles) the launch for `d`
 * reads.  Legal: the nine taps of a 3x3 window, kmode 0, unit strides, out_oy = out_ox = 0, C1 % 32 == 0, C2 % 32 == 0,
 * Cout % 64 == 0, GW >= 17, 16-byte aligned in1 / in2 / w / bias / res / out with ld % 4 == 0, inputs below 4 GiB, act none /
 * ReLU / leaky ReLU, and bnpart, ws, parity_merge, in_scale, bwd_x unset (w_split is not read).  d->w stays the fp32 packed
 * matrix (the non-finite path reads it).
 * ssg_pack_weights_bf16x1(d->w rows [R][Kp] in kmode 0, R, Kp, BN = that code): ssg_pack_weights_bf16x1_bytes bytes, layout
 * [R/bn][Kp/32 steps = chunk32 * 9 + tap][bn/16 fragments][64 lanes][16 B] (bn = BN - 1000; R % bn == 0, Kp % 288 == 0) -- the
 * 1128 / 1064 layout of ssg_pack_weights_split_bf16x3 with one plane, a third of its bytes.
 * ssg_conv2d_bf16x1_f32 validates on the host and returns a status before any launch.
 * ssg_conv2d_bf16x1_kernel_id: 70 / 71 = conv_halo_k32_x1_kernel<128> / <64> (profiling labels), SSG_EINVAL where refused. */
int ssg_conv2d_bf16x1_ok(const ssg_conv_desc* d);
int ssg_conv2d_bf16x1_kernel_id(const ssg_conv_desc* d);
int ssg_conv2d_bf16x1_f32(const ssg_conv_desc* d, const void* w_bf16x1, void* stream);
int64_t ssg_pack_weights_bf16x1_bytes(int R, int Kp, int BN);
int ssg_pack_weights_bf16x1(const float* w_packed, int R, int Kp, int BN, void* out, void* stream);

/* Opt-in bf16x2 convolution (conv_halo_k32_bf16.hip; ops.conv2d(..., precision='bf16x2')): the 3x3 stride-1 pad-1 conv (forward, and
 * the input gradient as the same conv on dout with the transposed pack) with each operand split ONCE into two bf16 terms,
 * x1 = bf16_rne(x), x2 = bf16_rne(x - x1), and three v_mfma_f32_16x16x32_bf16 per product in a fixed order, small terms first:
 * x1 w2, x2 w1, x1 w1 (x2 w2 is dropped).  fp32 accumulation, epilogue and tensors.  An APPROXIMATION: |error| <= (3 * 2^-16 +
 * 3 * 2^-32) * conv(|x|, |w|) from the dropped products, plus fp32 accumulation; half the matrix instructions of the fp32-class
 * kernel.  Never selected by ssg_conv2d_f32 or ssg_conv2d_bf16x1_f32: the caller launches it by name.  The summation order does
 * not depend on the grid.  Non-finite results are those of the fp32 kernels: an infinite (or bf16-overflowing, >= ~3.39e38)
 * operand makes its second term a NaN, and a tile that holds a non-finite accumulator is recomputed in fp32.
 * ssg_conv2d_bf16x2_ok: 0, or the pack format code (2128 / 2064 = 8 x 32-pixel x 128- / 64-channel tiles) the launch for `d`
 * reads.  Legal: what ssg_conv2d_bf16x1_ok takes (the nine taps of a 3x3 window, kmode 0, unit strides, out_oy = out_ox = 0,
 * C1 % 32 == 0, C2 % 32 == 0, Cout % 64 == 0, GW >= 17, 16-byte aligned pointers with ld % 4 == 0, inputs below 4 GiB, act none /
 * ReLU / leaky ReLU, and bnpart, ws, parity_merge, in_scale, bwd_x unset).  d->w stays the fp32 packed matrix (the non-finite
 * path reads it).
 * ssg_pack_weights_bf16x2(d->w rows [R][Kp] in kmode 0, R, Kp, BN = that code): ssg_pack_weights_bf16x2_bytes bytes, layout
 * [R/bn][Kp/32 steps = chunk32 * 9 + tap][2 planes][bn/16 fragments][64 lanes][16 B] (bn = BN - 2000; R % bn == 0, Kp % 288 == 0):
 * plane 0 the rounded value, plane 1 the rounded residual; twice the bytes of the bf16x1 pack.
 * ssg_conv2d_bf16x2_f32 validates on the host and returns a status before any launch.
 * ssg_conv2d_bf16x2_kernel_id: 90 / 91 = conv_halo_k32_x2_kernel<128> / <64> (profiling labels), SSG_EINVAL where refused. */
int ssg_conv2d_bf16x2_ok(const ssg_conv_desc* d);
int ssg_conv2d_bf16x2_kernel_id(const ssg_conv_desc* d);
int ssg_conv2d_bf16x2_f32(const ssg_conv_desc* d, const void* w_bf16x2, void* stream);
int64_t ssg_pack_weights_bf16x2_bytes(int R, int Kp, int BN);
int ssg_pack_weights_bf16x2(const float* w_packed, int R, int Kp, int BN, void* out, void* stream);

/* Opt-in bf16x1 kernels for the 3x3 STRIDE-2 pad-1 conv (models_seg_gan.py:37-39, the discriminator's s2 blocks) and its input
 * gradient (conv_s2_k32_x1.hip; ops.conv2d(..., precision='bf16x1')): the contract of ssg_conv2d_bf16x1_f32 -- operands rounded once
 * to bf16, fp32 accumulation, fp32 tensors, non-finite results those of the fp32 kernels -- with one input (C2 = 0) and no res.
 * ssg_conv2d_bf16x1_s2_*: the forward.  Legal: the nine row-major taps (dy = t / 3 - 1, dx = t % 3 - 1), kmode 0, in_sy = in_sx = 2,
 * out_s* = 1, out_o* = 0, C1 % 32 == 0, Cout % 64 == 0, Kp = 9 C1, GW >= 17, any H / W, 16-byte alignment, ld % 4 == 0, input below
 * 4 GiB, act none / ReLU / leaky ReLU, optional bias; bnpart, ws, parity_merge, in_scale, bwd_x, res unset.  The pack is
 * ssg_pack_weights_bf16x1's.  Kernel ids 73 / 74 = conv_s2_k32_x1_kernel<128,9> / <64,9> (4 x 32-pixel tiles).
 * ssg_conv2d_bf16x1_cls_*: ONE parity class of the input gradient, a launch of the per-class form of `parity_merge` above: ntaps =
 * 1 / 2 / 4 distinct taps with dy, dx in {0, +1}, in_s* = 1, out_sy = out_sx = 2, out_oy / out_ox in {0, 1}, in1 = dy (C1 % 32 == 0),
 * Cout = gradient rows (% 64 == 0), Kp = ntaps * C1, GW >= 17, (GH - 1) * 2 + out_oy < OH (and the same in x).  The pack is
 * ssg_pack_weights_bf16x1_taps(d->w rows [R][Kp] in kmode 0 with `ntaps` taps, R, Kp, ntaps, BN = the code _cls_ok returned):
 * layout [R/bn][Kp/32 steps = chunk32 * ntaps + tap][bn/16 fragments][64 lanes][16 B] (Kp % (32 ntaps) == 0).  Kernel ids 75 / 76,
 * 77 / 78, 79 / 80 = conv_s2_k32_x1_kernel<128 / 64> with 1, 2, 4 taps (8 x 32-pixel tiles).
 * Both launchers validate on the host and return a status before any launch; _ok returns 0 or the pack format code (1128 / 1064). */
int ssg_conv2d_bf16x1_s2_ok(const ssg_conv_desc* d);
int ssg_conv2d_bf16x1_s2_kernel_id(const ssg_conv_desc* d);
int ssg_conv2d_bf16x1_s2_f32(const ssg_conv_desc* d, const void* w_bf16x1, void* stream);
int ssg_conv2d_bf16x1_cls_ok(const ssg_conv_desc* d);
int ssg_conv2d_bf16x1_cls_kernel_id(const ssg_conv_desc* d);
int ssg_conv2d_bf16x1_cls_f32(const ssg_conv_desc* d, const void* w_bf16x1, void* stream);
int64_t ssg_pack_weights_bf16x1_taps_bytes(int R, int Kp, int ntaps, int BN);
int ssg_pack_weights_bf16x1_taps(const float* w_packed, int R, int Kp, int ntaps, int BN, void* out, void* stream);

/* Launches whose pixel-tile count leaves most of the chip idle (the 16x16 / 32x32 levels of archs.py:583-589, the
 * Cout <= 64 input gradients of SPADE's gamma|beta conv normalization.py:94-96, batch-1 inference api.py:322) split the
 * reduction over 16-channel chunks into slabs; an ordered second stage adds the slabs and applies bias / res / act
 * (bitwise reproducible).  Returns 0 when the launch for `d` would not split. */
int64_t ssg_conv2d_workspace_bytes(const ssg_conv_desc* d);

int ssg_conv2d_igemm_f32(const ssg_conv_desc* d, void* stream);
/* Dispatching entry point (what the host side calls): convs with <= 8 channels on one side and
 * unit strides (SPADE's C->3->h->C chain normalization.py:90-96, the 3-channel image / logit /
 * mask layers archs.py:210,615, models_seg_gan.py:37) run on HBM-bound VALU kernels; everything
 * else goes to the MFMA implicit GEMM above.  Same descriptor, same semantics.
 * ssg_conv2d_kernel_id: the kernel ssg_conv2d_f32 launches for the descriptor as given (w_split, in_scale, bnpart and ws
 * included; profiling labels):
 *   0..2 = conv_igemm_kernel<128,128>/<256,64>/<256,32> (register-staged),
 *   10 = thin small-Cout (VALU), 12/13 = thin4 kernels on the 4x4x1 MFMA (4-channel input / Cout <= 8 with Cin % 64 == 0),
 *   14 = tiny4 (4 -> <= 8 channels, VALU), 15 = thin32 (4-channel input, 3x3, Cout >= 32 on the 32x32x2 MFMA),
 *   16 = conv1x1_k64 (streaming 1x1, 64 input channels),
 *   20/21/22 = conv_igemm_dma_kernel<128,128>/<256,64>/<128,64> (LDS-DMA pipeline, Cin % 16 == 0 and Cout > 32),
 *   30/31/32 = conv_igemm_halo_kernel<128,128>/<256,64>/<128,64> (LDS-resident halo tile: the 9 taps of a 3x3 window at unit
 *   stride), 33/34 = conv_igemm_halo16_kernel<128,128>/<128,64> (the same on 8x16-pixel tiles, images <= 16 wide),
 *   split operands (w_split): 40/41 = conv_igemm_halo_x3_kernel<128,128>/<128,64>, 42 = the merged parity classes
 *   (conv_igemm_halo_x3_kernel<128,64,4,1,true>), 50/51 = conv_igemm_dma_x3_kernel<64>/<128>,
 *   60..64 = conv_halo_k32_kernel<8,128>/<4,64>/<16,64>/<8,16>/<8,32> (pack formats 1128 / 1064 / 1064 / 1016 / 1032). */
int ssg_conv2d_f32(const ssg_conv_desc* d, void* stream);
int ssg_conv2d_kernel_id(const ssg_conv_desc* d);
/* Rows of `bnpart` the launch for `d` writes, or 0 when the kernel `d` maps to has no statistics epilogue (the caller then
 * runs ssg_bn_stats_f32).  The batch norm that follows the conv (archs.py:211,213; models_seg_gan.py:43) takes its
 * (sum x, sum x^2) from these rows (ssg_bn_stats_from_partials_f32): one full read of the conv output less. */
int ssg_conv2d_bnpart_rows(const ssg_conv_desc* d);

/* Weight packing from the reference's OIHW parameter layout [O][I][KH][KW] (the
 * state_dict layout of nn.Conv2d, archs.py:210 etc.) into the [R][Kp] operand above.
 *   transpose = 0: rows R = O, reduce over I  (forward)
 *   transpose = 1: rows R = I, reduce over O  (input gradient)
 * tap t reads kernel position (ky[t], kx[t]).  `Cred_pad` is the reduced-channel count
 * rounded up to a multiple of 4 (pad channels get zero weights). */
int ssg_pack_weights_f32(const float* w_oihw, int O, int I, int KH, int KW,
                         int transpose, int ntaps, const int* ky, const int* kx,
                         int kmode, int Cred_pad, int Kp, float* out, void* stream);
/* The same with every weight multiplied by 1 / *sigma (device scalar): a spectrally normalised conv (spectral_norm.py:86-88)
 * packs `weight_orig` with its sigma, so W / sigma is never materialised in OIHW form. */
int ssg_pack_weights_scaled_f32(const float* w_oihw, int O, int I, int KH, int KW,
                                int transpose, int ntaps, const int* ky, const int* kx,
                                int kmode, int Cred_pad, int Kp, const float* sigma, float* out, void* stream);

/* Weight gradient (replaces conv2d's weight-grad at the same call sites).
 *   dw[co, c, ky[t], kx[t]] = sum_{n,gy,gx} dout[n,gy,gx,co] * in[n, gy*in_sy+dy[t], gx*in_sx+dx[t], c]
 * Two deterministic stages: split-K partial slabs into `ws`, then an ordered reduce that
 * writes the OIHW gradient (only c < Cin_real channels; pad channels are dropped).
 * The bias gradient is ssg_channel_sum_f32 over dout. */
typedef struct {
  const float* in1; const float* in2; int C1, C2, ld1, ld2;
  int N, H, W;
  const float* dout; int Cout, ldd; int GH, GW;
  int in_sy, in_sx;
  int ntaps; int dy[SSG_MAX_TAPS]; int dx[SSG_MAX_TAPS]; int ky[SSG_MAX_TAPS]; int kx[SSG_MAX_TAPS];
  int KH, KW, Cin_real;
  float* dw_oihw;           /* [Cout][Cin_real][KH][KW] */
  float* ws; int64_t ws_bytes;
  int flags;                /* bit 0: 3x3 stride-1 weight gradients multiply on the bf16 matrix pipe with both fp32 operands split into
                             * three bf16 terms (wgrad_halo_x3_kernel: fp32-class accuracy, see ssg_conv_desc.w_split); 0 = fp32 MFMA */
  /* ABI 8: the x operand is act_in(in1 * in_scale[c] + in_shift[c]) (see ssg_conv_desc.in_scale): the weight gradient of a conv
   * whose input was a fused batch-norm apply.  NULL = off; only where ssg_conv2d_wgrad_in_affine_ok(d) returns 1. */
  const float* in_scale; const float* in_shift; int in_act; float in_slope;
} ssg_wgrad_desc;

int64_t ssg_conv2d_wgrad_workspace_bytes(const ssg_wgrad_desc* d);
int ssg_conv2d_wgrad_in_affine_ok(const ssg_wgrad_desc* d);   /* ABI 8 */
int ssg_conv2d_wgrad_f32(const ssg_wgrad_desc* d, void* stream);
/* 2 = wgrad_kernel<128,32> (Cout <= 32), 20/21 = wgrad_dma_kernel<128,128>/<128,64> (Cout > 64 / > 32), 30/31 =
 * wgrad_halo_kernel<32,128>/<64,64> (3x3 stride-1 window kept in LDS, channel counts multiples of 32 / 64), 40/41 and 50/51 =
 * the split-operand (x3) forms of 30/31 and 20/21 (flags bit 0), 60 = wgrad_k32_kernel (below), 15/16 = wgrad4_kernel (4x4x1
 * MFMA: dout <= 4 channels / in = 4 channels), 17 = wgrad_tiny4_kernel (in = 4 channels, dout <= 8, 3x3; VALU), 18 =
 * wgrad32_cin_kernel (in = 4 channels, 3x3, Cout >= 32 on >= 65536 pixels; 32x32x2 MFMA).  No other id is returned: Cout > 32
 * always takes the DMA or halo kernels (no 0/1), and a thin plan is 10 + ssg_wgrad4_kind with kinds 5..8 (no 13/14). */
int ssg_conv2d_wgrad_kernel_id(const ssg_wgrad_desc* d);
/* 60 = wgrad_k32_kernel (conv_wgrad_k32.hip, round 4): the split-operand weight gradient of 3x3 stride-1 convs on
 * v_mfma_f32_16x16x32_bf16 (64-channel multiples on every side; flags bit 0).  ssg_wgrad_set_k32_mode(0 / 1) switches it off / on
 * at run time (default on, SSG_WGRAD_K32). */
int ssg_wgrad_set_k32_mode(int mode);

/* Opt-in bf16x1 weight gradient (conv_wgrad_k32_bf16.hip; ops.train_precision('bf16x1')): the contract of ssg_conv2d_wgrad_f32 for the
 * 3x3 stride-1 pad-1 conv, with both operands rounded once to bf16 (round to nearest even) and fp32 accumulation -- one MFMA per
 * product instead of six.  An APPROXIMATION: |error| <= (2^-8 + 2^-18) * sum |in| |dout| plus the fp32 accumulation error;
 * ssg_conv2d_wgrad_f32 never routes here.  A workgroup that meets a non-finite accumulator (an fp32 value >= 2^128 - 2^119 rounds
 * to bf16 infinity) recomputes its tile from the fp32 operands, so the result class is that of the fp32 kernel.
 * ssg_conv2d_wgrad_bf16x1_ok: 1 where the launch takes `d` -- the nine row-major taps (dy = t / 3 - 1, dx = t % 3 - 1, ky = t / 3,
 *   kx = t % 3) at unit stride over the whole image (GH == H, GW == W), C1 % 64 == C2 % 64 == Cout % 64 == 0, Cin_real == C1 + C2,
 *   GW >= 17, pixel strides multiples of 4, tensors within 32-bit byte offsets, in_scale == NULL -- else 0.  Pointers are not read.
 * ssg_conv2d_wgrad_bf16x1_workspace_bytes: bytes of d->ws for the split-K slabs (0 where refused).
 * ssg_conv2d_wgrad_bf16x1_f32 validates on the host and returns a status before any launch; d->flags is ignored.
 * ssg_conv2d_wgrad_bf16x1_kernel_id: 72 = wgrad_k32_x1_kernel (profiling label), SSG_EINVAL where refused. */
int ssg_conv2d_wgrad_bf16x1_ok(const ssg_wgrad_desc* d);
int64_t ssg_conv2d_wgrad_bf16x1_workspace_bytes(const ssg_wgrad_desc* d);
int ssg_conv2d_wgrad_bf16x1_f32(const ssg_wgrad_desc* d, void* stream);
int ssg_conv2d_wgrad_bf16x1_kernel_id(const ssg_wgrad_desc* d);

/* Opt-in bf16x2 weight gradient (conv_wgrad_k32_bf16.hip; precision 'bf16x2'): the contract, legal shapes, workspace and ordered
 * split-K reduction of the bf16x1 group above, with both operands (the x window and dout) split once into two bf16 terms and three
 * MFMAs per product, small terms first: x1 d2, x2 d1, x1 d1.  An APPROXIMATION: |error| <= (3 * 2^-16 + 3 * 2^-32) * sum |in| |dout|
 * plus the fp32 accumulation error; neither ssg_conv2d_wgrad_f32 nor ssg_conv2d_wgrad_bf16x1_f32 routes here.  A workgroup that
 * holds a non-finite accumulator (every one that read an infinite or bf16-overflowing operand) recomputes its tile in fp32.
 * ssg_conv2d_wgrad_bf16x2_ok: 1 where the launch takes `d` (the predicate of ssg_conv2d_wgrad_bf16x1_ok), else 0.
 * ssg_conv2d_wgrad_bf16x2_workspace_bytes: bytes of d->ws for the split-K slabs (0 where refused).
 * ssg_conv2d_wgrad_bf16x2_f32 validates on the host and returns a status before any launch; d->flags is ignored.
 * ssg_conv2d_wgrad_bf16x2_kernel_id: 92 = wgrad_k32_x2_kernel (profiling label), SSG_EINVAL where refused. */
int ssg_conv2d_wgrad_bf16x2_ok(const ssg_wgrad_desc* d);
int64_t ssg_conv2d_wgrad_bf16x2_workspace_bytes(const ssg_wgrad_desc* d);
int ssg_conv2d_wgrad_bf16x2_f32(const ssg_wgrad_desc* d, void* stream);
int ssg_conv2d_wgrad_bf16x2_kernel_id(const ssg_wgrad_desc* d);

/* Opt-in bf16x1 weight gradient of the 3x3 STRIDE-2 pad-1 conv (conv_wgrad_s2_k32_x1.hip; precision 'bf16x1' with wgrad_s2 'bf16x1'):
 * the contract, rounding, error bound and non-finite guard of the group above, dw[ky][kx][ci][co] = sum in[n, 2oy + ky - 1,
 * 2ox + kx - 1, ci] * dout[n, oy, ox, co].  A route of its own: neither ssg_conv2d_wgrad_f32 nor ssg_conv2d_wgrad_bf16x1_f32 comes here.
 * ssg_conv2d_wgrad_bf16x1_s2_ok: 1 where the launch takes `d` -- the nine row-major taps (dy = t / 3 - 1, dx = t % 3 - 1, ky = t / 3,
 *   kx = t % 3), in_sy == in_sx == 2, GH == (H + 1) / 2, GW == (W + 1) / 2, GW >= 17, C1 % 64 == 0, C2 == 0 (no concat),
 *   Cout % 64 == 0, Cin_real == C1, pixel strides multiples of 4, tensors within 32-bit byte offsets, in_scale == NULL -- else 0.
 *   Pointers are not read.
 * ssg_conv2d_wgrad_bf16x1_s2_workspace_bytes: bytes of d->ws for the split-K slabs (0 where refused).
 * ssg_conv2d_wgrad_bf16x1_s2_f32 validates on the host and returns a status ("wgrad bf16x1 s2: ..." in ssg_last_error) before any
 *   launch; d->flags is ignored.
 * ssg_conv2d_wgrad_bf16x1_s2_kernel_id: 81 / 82 = wgrad_s2_k32_x1_kernel<4> / <2> (128 / 64 output channels per workgroup, by
 *   Cout % 128), SSG_EINVAL where refused. */
int ssg_conv2d_wgrad_bf16x1_s2_ok(const ssg_wgrad_desc* d);
int64_t ssg_conv2d_wgrad_bf16x1_s2_workspace_bytes(const ssg_wgrad_desc* d);
int ssg_conv2d_wgrad_bf16x1_s2_f32(const ssg_wgrad_desc* d, void* stream);
int ssg_conv2d_wgrad_bf16x1_s2_kernel_id(const ssg_wgrad_desc* d);

/* Attention gate of AttUNet (archs.py:115-144, `x * psi`): y[p][c] = x[p][c] * sigmoid(g[p]) with one gate
 * logit per pixel (g is the 1-channel BatchNorm output, pixel stride ldg); the sigmoid is folded in.
 * backward: dx = dy * s, dg[p] = (sum_c dy*x) * s * (1 - s) (written as a 4-float pixel: value, 0, 0, 0). */
int ssg_pixel_gate_fwd_f32(const float* x, int ldx, const float* g, int ldg, int64_t P, int C, float* y, int ldy, void* stream);
int ssg_pixel_gate_bwd_f32(const float* x, int ldx, const float* g, int ldg, const float* dy, int lddy, int64_t P, int C,
                           float* dx, int lddx, float* dg, int lddg, void* stream);

/* Skinny fully-connected forward (replaces nn.Linear's forward at models_seg_gan.py:281-283, fc1/fc2 of the
 * discriminator): y[n][o] = act(sum_k x[n][k] * w[o][k] + bias[o]).  `w` is the parameter itself ([O][K] row
 * major, no packing); the weight matrix is streamed once (HBM-bound), K slices are summed in order by a
 * finishing kernel (deterministic).  k % 4 == 0, ldx % 4 == 0, x and w 16-B aligned.  The input and weight
 * gradients stay on ssg_conv2d_f32 / ssg_conv2d_wgrad_f32 (1x1 conv on a 1 x n image). */
int64_t ssg_linear_fwd_workspace_bytes(int n, int k, int o);
int ssg_linear_fwd_f32(const float* x, int n, int k, int ldx, const float* w, int o, const float* bias, int act,
                       float slope, float* y, int ldy, float* ws, int64_t ws_bytes, void* stream);
/* dw[o][k] = sum_n dy[n][o] * x[n][k] (the weight gradient of nn.Linear, models_seg_gan.py:281-283), contiguous [O][K] output,
 * summed over n in order; x rows of stride ldx (k % 4 == 0, 16-byte aligned), dy rows of stride ldd. */
int ssg_linear_wgrad_f32(const float* x, int n, int k, int ldx, const float* dy, int o, int ldd, float* dw, void* stream);

/* ------------------------------------------------------------------ bf16 pointwise convolution (BASELINE config 4)
 * SURVEY.md 8(b) `conv2d_{fwd,dgrad,wgrad}_nhwc_bf16` for the 1x1 layers of the EfficientNet MBConv blocks
 * (efficientnet_pytorch/model.py:40-58: _expand_conv, _project_conv; model.py:172 _conv_head): bf16 operands on
 * v_mfma_f32_32x32x16_bf16, fp32 accumulation.  bf16 activations are NHWC-with-stride tensors of 16-bit elements whose
 * channel count and pixel stride are multiples of 8 (16-byte rows).  Weights stay fp32 in the module; per use they are
 * packed to bf16 rows [rows_pad][Kp] (rows_pad % 128 == 0, Kp % 32 == 0, zero padded): transpose 0 = [O][I] for the
 * forward, transpose 1 = [I][O] for the input gradient.  ssg_pack_weights_bf16 rounds to nearest even and writes all
 * rows_pad x Kp elements: +0 in every row past the matrix and in columns [cols, Kp) of every row.
 *   ssg_gemm_bf16        out[p][n] = sum_k x[p][k] * w[n][k] (+ res[p][n]), out/res bf16      (forward and dgrad)
 *                        w_packed: N rows of stride Kp (Kp >= K); columns [K, round32(K)) must be zero (the pack's
 *                        padding), rows >= N are never read.  x, res and out are read / written in channels [0, K) /
 *                        [0, N) only, whatever ldx, ldr, ldo.  res == NULL: no residual, ldr is ignored (any value).
 *   ssg_gemm_wgrad_bf16  dw[m][n]  = sum_p dy[p][m] * x[p][n], fp32 [M][N] (= OIHW of a 1x1 conv); split-K over pixels
 *                        with fp32 slabs in `ws` and an ordered reduce (bitwise reproducible) */
int ssg_pack_weights_bf16(const float* w, int O, int I, int transpose, int rows_pad, int Kp, void* out, void* stream);
int ssg_gemm_bf16(const void* x, int64_t P, int K, int ldx, const void* w_packed, int Kp, int N,
                  const void* res, int ldr, void* out, int ldo, void* stream);
int64_t ssg_gemm_wgrad_bf16_workspace_bytes(int64_t P, int M, int N);
int ssg_gemm_wgrad_bf16(const void* dy, int ldd, const void* x, int ldx, int64_t P, int M, int N, float* dw,
                        void* ws, int64_t ws_bytes, void* stream);

/* bf16 dense k x k conv of a <= 4-channel image (the EfficientNet stem, efficientnet_pytorch/model.py:162,206: 3 -> 32..48, k = 3, s = 2,
 * TF-SAME padding utils.py:123-146): SURVEY.md 8(b) `conv2d_{fwd,dgrad,wgrad}_nhwc_bf16`, k = 3.  x: fp32 NHWC image with 4-channel pixel
 * rows (the model input); image values and weights are rounded to bf16 before they multiply, fp32 accumulation, bf16 output [N, OH, OW, Cout]
 * (Cout % 8 == 0).  w_oihw / dw_oihw: fp32 [Cout][Cin][KH][KW].  wgrad: ws of ssg_conv2d_thin_bf16_wgrad_workspace_bytes bytes.
 * dgrad writes the fp32 image gradient as 4-float pixels of stride lddx: channels [0, Cin) the gradient, channels [Cin, 4) zeros,
 * lanes [4, lddx) untouched.  The forward and the weight gradient load all 4 floats of an image pixel (channels [Cin, 4) must be
 * finite: they meet zero weights / are dropped) and nothing of lanes [4, ldx). */
int ssg_conv2d_thin_bf16(const float* x, int N, int H, int W, int ldx, const float* w_oihw, int Cout, int Cin, int KH, int KW,
                         int stride, int pad_t, int pad_l, int OH, int OW, void* y, int ldy, void* stream);
int64_t ssg_conv2d_thin_bf16_wgrad_workspace_bytes(int N, int OH, int OW, int Cout, int KH, int KW);
int ssg_conv2d_thin_bf16_wgrad(const float* x, int N, int H, int W, int ldx, const void* dy, int lddy, int Cout, int Cin,
                               int KH, int KW, int stride, int pad_t, int pad_l, int OH, int OW, float* dw_oihw, void* ws,
                               void* stream);
int ssg_conv2d_thin_bf16_dgrad(const void* dy, int lddy, int N, int H, int W, const float* w_oihw, int Cout, int Cin, int KH, int KW,
                               int stride, int pad_t, int pad_l, int OH, int OW, float* dx, int lddx, void* stream);

/* bf16 twins of the HBM-bound kernels the MBConv block needs (same arguments and arithmetic as their _f32 namesakes below:
 * tensors are bf16 in HBM, arithmetic is fp32 in registers, statistics fp64; C % 4 == 0, 8-byte loads per lane).
 * Batch norm with act = SSG_ACT_SWISH fuses `swish(bn(x))` (model.py:75,80) into the apply pass; its backward recomputes the
 * pre-activation from x and (scale, shift) (y must be NULL), so the BN output before the swish is never stored. */
int ssg_bn_stats_bf16(const void* x, int64_t P, int C, int ld, double* sums, int with_count, void* ws, void* stream);
int ssg_bn_apply_bf16(const void* x, int64_t P, int C, int ld, const float* scale, const float* shift,
                      const void* res, int ldr, int act, float slope, void* y, int ldy, void* stream);
int ssg_bn_bwd_reduce_bf16(const void* x, const void* y, const void* dy, int64_t P, int C, int ldx, int ldy, int lddy,
                           const float* mean, const float* invstd, const float* scale, const float* shift,
                           int act, float slope, double* sums, int with_count, void* ws, void* stream);
int ssg_bn_bwd_apply_bf16(const void* x, const void* y, const void* dy, int64_t P, int C, int ldx, int ldy, int lddy,
                          const float* mean, const float* invstd, const float* weight, const float* scale, const float* shift,
                          const double* sums, double count, int act, float slope, void* dx, int lddx, void* dres, int lddres,
                          float* dweight, float* dbias, void* stream);
int ssg_dwconv2d_fwd_bf16(const void* in, int N, int H, int W, int C, int ld, const float* w, const float* bias, int KH, int KW,
                          int stride, int pad_top, int pad_left, int OH, int OW, void* out, int ldo, void* stream);
int ssg_dwconv2d_dgrad_bf16(const void* dout, int lddo, int N, int H, int W, int C, const float* w, int KH, int KW, int stride,
                            int pad_top, int pad_left, int OH, int OW, void* dx, int lddx, void* stream);
int ssg_dwconv2d_wgrad_bf16(const void* in, int N, int H, int W, int C, int ld, const void* dout, int lddo, int KH, int KW,
                            int stride, int pad_top, int pad_left, int OH, int OW, float* dw, void* ws, void* stream);
int ssg_channel_scale_fwd_bf16(const void* x, int ldx, const float* s, int N, int64_t S, int C, void* y, int ldy, void* stream);
int ssg_sample_channel_sum_bf16(const void* a, int lda, const void* b, int ldb, int N, int64_t S, int C, float scale,
                                float* out, void* ws, void* stream);
int ssg_broadcast_rows_bf16(const float* s, int N, int64_t S, int C, float scale, void* y, int ldy, void* stream);
int ssg_add_bf16(const void* a, int lda, const void* b, int ldb, int64_t P, int C, void* out, int ldo, void* stream);
int ssg_convert_f32_to_bf16(const float* src, int ldsrc, int64_t P, int C, void* dst, int lddst, void* stream);
int ssg_convert_bf16_to_f32(const void* src, int ldsrc, int64_t P, int C, float* dst, int lddst, void* stream);

/* ------------------------------------------------------------------ layout helpers
 * NCHW (the reference's layout at the boundary: dataset.py:144 tensors, G logits) <->
 * internal NHWC-with-stride.  Pad channels [C, ld) are written as 0. */
int ssg_nchw_to_nhwc_f32(const float* src, int N, int C, int H, int W, float* dst, int ld, void* stream);
int ssg_nhwc_to_nchw_f32(const float* src, int ld, int N, int C, int H, int W, float* dst, void* stream);

/* ------------------------------------------------------------------ batch norm (HBM-bound)
 * Training-mode BatchNorm2d (archs.py:211,213; models_seg_gan.py:43), eps/momentum as the
 * module holds them.  Split so a cross-rank all-reduce of the partial sums (sync-BN,
 * batchnorm.py:63-64,104-107) fits between stage 1 and stage 2.
 *   stage 1: sums[0:C] = sum_p x[p,c], sums[C:2C] = sum_p x[p,c]^2  (fp64, deterministic)
 *   stage 2: mean, invstd; scale = w*invstd, shift = b - mean*scale; running stats update
 *            var_mode 0: invstd = 1/sqrt(var_b + eps)        (torch, batchnorm.py:52-55)
 *            var_mode 1: invstd = clamp(var_b, eps)^-1/2     (sync branch, batchnorm.py:127)
 *   apply  : y = x*scale[c] + shift[c] (+res) -> act
 * Sync-BN with unequal local batches: with_count != 0 makes stage 1 also write sums[2C] = P (so `sums` holds 2C+1
 * doubles and the rank's pixel count is all-reduced with the sums); stage 2 and the backward apply take the count from
 * sums[2C] when their `count` argument is <= 0.
 */
int64_t ssg_bn_workspace_bytes(int64_t P, int C);
int ssg_bn_stats_f32(const float* x, int64_t P, int C, int ld, double* sums, int with_count, void* ws, void* stream);
/* stage 1 from the conv epilogue's per-tile rows (ssg_conv_desc.bnpart); count > 0 also writes sums[2C] = count */
int64_t ssg_bn_stats_from_partials_workspace_bytes(int rows, int C);
int ssg_bn_stats_from_partials_f32(const double* part, int rows, int C, double* sums, double count, void* ws, void* stream);
int ssg_bn_finalize_f32(const double* sums, double count, int C, const float* weight, const float* bias,
                        float eps, float momentum, int var_mode,
                        float* running_mean, float* running_var,
                        float* mean, float* invstd, float* scale, float* shift, void* stream);

/* Local (un-synchronised) batch norm in one call: the statistics passes finish with the per-channel constants and the running
 * estimates of ssg_bn_finalize_f32 (same arithmetic, same bits), one launch less per batch-norm forward
 * (archs.py:211,213, models_seg_gan.py:43, efficientnet_pytorch/model.py:75,80,90).  `count` of the from-partials form =
 * pixels the partial rows cover. */
typedef struct ssg_bn_fin {
  const float* weight; const float* bias;     /* may be NULL (1 / 0) */
  float eps, momentum; int var_mode;          /* var_mode as ssg_bn_finalize_f32 */
  float* running_mean; float* running_var;    /* may be NULL */
  float* mean; float* invstd; float* scale; float* shift;
} ssg_bn_fin;
int ssg_bn_stats_finalize_f32(const float* x, int64_t P, int C, int ld, const ssg_bn_fin* fin, void* ws, void* stream);
int ssg_bn_stats_finalize_bf16(const void* x, int64_t P, int C, int ld, const ssg_bn_fin* fin, void* ws, void* stream);
int ssg_bn_stats_from_partials_finalize_f32(const double* part, int rows, int C, double count, const ssg_bn_fin* fin, void* ws, void* stream);
int ssg_bn_apply_f32(const float* x, int64_t P, int C, int ld, const float* scale, const float* shift,
                     const float* res, int ldr, int act, float slope, float* y, int ldy, void* stream);
/* backward: g = dy masked by the activation (y>0 ? 1 : slope), dres = g (if wanted);
 *   stage 1: sums[0:C] = sum g, sums[C:2C] = sum g*xhat   (fp64; all-reduced for sync-BN)
 *   apply  : dx = scale*(g - sums0/count - xhat*sums1/count); dweight = sums1, dbias = sums0
 * The activation mask comes from the saved output y, or -- y = NULL, for a forward WITHOUT residual -- is
 * recomputed from x with the (scale, shift) the forward used (one tensor read less per kernel). */
int ssg_bn_bwd_reduce_f32(const float* x, const float* y, const float* dy, int64_t P, int C,
                          int ldx, int ldy, int lddy, const float* mean, const float* invstd,
                          const float* scale, const float* shift,
                          int act, float slope, double* sums, int with_count, void* ws, void* stream);
int ssg_bn_bwd_apply_f32(const float* x, const float* y, const float* dy, int64_t P, int C,
                         int ldx, int ldy, int lddy, const float* mean, const float* invstd,
                         const float* weight, const float* scale, const float* shift,
                         const double* sums, double count, int act, float slope,
                         float* dx, int lddx, float* dres, int lddres,
                         float* dweight, float* dbias, void* stream);
/* 1-bit activation masks.  Where the forward had a residual, the backward needs of y only the sign: ssg_bn_apply_mask_f32 is
 * ssg_bn_apply_f32 (same y, bit for bit) that also writes mask[p][c / 8] bit c % 8 = (y[p][c] > 0), tested on the stored value
 * (uint8, row stride ldm >= C / 8 bytes), and the _mask forms of the two backward passes read those bytes where the plain ones
 * read y: 1/32 of the bytes, the same sums, dx, dres, dweight and dbias bit for bit.
 * ssg_bn_mask_ok(C, act): 1 where the forms apply -- C % 8 == 0 and act ReLU or LeakyReLU (fp32 tensors only); they return
 * SSG_EINVAL for anything else. */
int ssg_bn_mask_ok(int C, int act);
int ssg_bn_apply_mask_f32(const float* x, int64_t P, int C, int ld, const float* scale, const float* shift,
                          const float* res, int ldr, int act, float slope, float* y, int ldy,
                          uint8_t* mask, int ldm, void* stream);
int ssg_bn_bwd_reduce_mask_f32(const float* x, const uint8_t* mask, const float* dy, int64_t P, int C,
                               int ldx, int ldm, int lddy, const float* mean, const float* invstd,
                               int act, float slope, double* sums, int with_count, void* ws, void* stream);
int ssg_bn_bwd_apply_mask_f32(const float* x, const uint8_t* mask, const float* dy, int64_t P, int C,
                              int ldx, int ldm, int lddy, const float* mean, const float* invstd,
                              const float* weight, const double* sums, double count, int act, float slope,
                              float* dx, int lddx, float* dres, int lddres,
                              float* dweight, float* dbias, void* stream);
/* ssg_bn_bwd_apply_f32 in the block geometry of the column reducers, which also returns dxsum[c] = sum_p dx[p][c] with the bits
 * of ssg_channel_sum_f32(dx): the bias gradient of the conv in front of the batch norm, without a pass over the fresh dx.
 * The activation mask comes from `mask` (1-bit form), else from y, else (both NULL) is recomputed from x with (scale, shift).
 * act: none, ReLU or LeakyReLU.  dx is required; ws: ssg_bn_workspace_bytes(P, C) bytes. */
int ssg_bn_bwd_apply_sums_f32(const float* x, const float* y, const uint8_t* mask, const float* dy, int64_t P, int C,
                              int ldx, int ldy, int ldm, int lddy, const float* mean, const float* invstd,
                              const float* weight, const float* scale, const float* shift,
                              const double* sums, double count, int act, float slope,
                              float* dx, int lddx, float* dres, int lddres,
                              float* dweight, float* dbias, float* dxsum, void* ws, void* stream);
/* eval-mode / generic per-channel affine: y = x*scale + shift -> act (also used for bias+act) */
/* Backward of a batch norm whose statistics are CONSTANTS (eval mode / frozen: torch.nn.functional.batch_norm(training=False),
 * archs.py:211,213 under model.eval()), in one pass -- no per-batch mean to subtract, so the stores ride the reduction sweep:
 *   g = dy * act'(.)   mask from the saved output y, or -- y = NULL, forward without residual -- recomputed as
 *                      x*scale + shift with the forward's own fma (ReLU / LeakyReLU); swish: derivative at x*scale + shift
 *   dx   = g * scale[c]         (scale = NULL: dx = g;  dx = NULL: not written)
 *   dres = g                    (dres = NULL: not written)
 *   sums[0:C] = sum_p g,  sums[C:2C] = sum_p g * (x - mean[c]) * invstd[c]   (mean = invstd = NULL: second half written as 0, x may be NULL)
 * fp64 partial rows, fixed order, no atomics: sums carry the bits of ssg_bn_bwd_reduce_f32 on the same inputs.
 * ws: ssg_bn_workspace_bytes(P, C) bytes.  C % 4 == 0; every row stride is its own (channel slices, pad lanes).
 * With x = mean = scale = NULL: activation backward + bias gradient of a conv epilogue in one read of dy. */
int ssg_bn_frozen_bwd_f32(const float* x, const float* y, const float* dy, int64_t P, int C, int ldx, int ldy, int lddy,
                          const float* mean, const float* invstd, const float* scale, const float* shift, int act, float slope,
                          float* dx, int lddx, float* dres, int lddres, double* sums, void* ws, void* stream);
/* Gradients through the fold of a frozen batch norm into its conv: Wf[o] = W[o]*s[o], bf[o] = beta[o] - mean[o]*s[o], s = gamma*invstd.
 * Per output channel o, K = Cin*kh*kw:  t = sum_k dwf[o,k]*w[o,k] (fp64, fixed order)
 *   dw[o,k] = dwf[o,k]*s[o];   dgamma[o] = (t - mean[o]*sums_g[o]) * invstd[o];   dbeta[o] = sums_g[o]     (each stored once, from fp64)
 * sums_g = sum_p of the gradient at the conv output (ssg_bn_frozen_bwd_f32's sums[0:C]).  dw may be NULL, and so may the pair
 * dgamma / dbeta (w, mean, invstd, sums_g are then not read). */
int ssg_bn_fold_bwd_f32(const float* dwf, const float* w, int Cout, int64_t K, const float* s, const float* mean,
                        const float* invstd, const double* sums_g, float* dw, float* dgamma, float* dbeta, void* stream);

/* ------------------------------------------------------------------ pool / unpool / upsample
 * MaxPool2d(2,2,return_indices) archs.py:571,628-643; MaxUnpool2d(2,2) archs.py:572,648-659;
 * Upsample(x2, bilinear, align_corners=True) archs.py:573,664,667.  The window argmax is kept
 * as one byte (0..3 = dy*2+dx) per output element; ties resolve to the first in scan order
 * and NaN wins, as ATen's CPU max_pool2d does. */
int ssg_maxpool2x2_fwd_f32(const float* x, int N, int H, int W, int C, int ldx, float* y, int ldy, uint8_t* idx, void* stream);
int ssg_maxpool2x2_bwd_f32(const float* dy, int lddy, const uint8_t* idx, int N, int H, int W, int C, float* dx, int lddx, void* stream);
/* dx = res + maxpool backward(dy): the gradient of an encoder output that feeds both the pool and a skip connection
 * (archs.py:628-667) in one pass; res is laid out like dx. */
int ssg_maxpool2x2_bwd_add_f32(const float* dy, int lddy, const uint8_t* idx, const float* res, int ldr, int N, int H, int W, int C,
                               float* dx, int lddx, void* stream);
int ssg_maxunpool2x2_fwd_f32(const float* x, int ldx, const uint8_t* idx, int N, int OH, int OW, int C, float* y, int ldy, void* stream);
int ssg_maxunpool2x2_bwd_f32(const float* dy, int lddy, const uint8_t* idx, int N, int OH, int OW, int C, float* dx, int lddx, void* stream);
int ssg_upsample2x_bilinear_fwd_f32(const float* x, int N, int H, int W, int C, int ldx, float* y, int ldy, void* stream);
int ssg_upsample2x_bilinear_bwd_f32(const float* dy, int lddy, int N, int H, int W, int C, float* dx, int lddx, void* stream);
int ssg_upsample2x_nearest_fwd_f32(const float* x, int N, int H, int W, int C, int ldx, float* y, int ldy, void* stream);
int ssg_upsample2x_nearest_bwd_f32(const float* dy, int lddy, int N, int H, int W, int C, float* dx, int lddx, void* stream);
/* AdaptiveAvgPool2d((6,6)) + flatten in NCHW order (models_seg_gan.py:277,294-295):
 * y[n, c*36 + oy*6 + ox]. */
int ssg_adaptive_avgpool_flat_fwd_f32(const float* x, int N, int H, int W, int C, int ldx, int OHW, float* y, void* stream);
int ssg_adaptive_avgpool_flat_bwd_f32(const float* dy, int N, int H, int W, int C, int OHW, float* dx, int lddx, void* stream);

/* ------------------------------------------------------------------ elementwise
 * SPADE modulate out = x*(1+gamma)+beta (normalization.py:120) and its gradients
 * dx = dy*(1+gamma), dgamma = dy*x, dbeta = dy.  gb holds gamma in channels [0,C) and beta
 * in [C,2C) of one 2C-channel tensor (the fused gamma|beta conv output). */
/* SPADE with the gamma|beta conv and the modulation in ONE kernel (normalization.py:117-120): `d` describes the 3x3 conv from the
 * 4-channel (padded) activation to 2C channels whose packed weight rows are [gamma 0..C-1 | beta C..2C-1] (bias likewise, no
 * residual / activation), but d->out receives  x * (1 + gamma) + beta  (C channels, pixel stride d->ldo) and `gamma` (incl. its
 * bias; pixel stride ldg) is kept for the backward pass; the [N,2C,H,W] tensor never exists.  ssg_spade_conv_modulate_ok(d):
 * 1 when this shape runs on the fused kernel (4-channel input, 3x3, >= 65536 pixels), else the caller runs ssg_conv2d_f32 +
 * ssg_spade_modulate_fwd_f32. */
int ssg_spade_conv_modulate_ok(const ssg_conv_desc* d);
int ssg_spade_conv_modulate_f32(const ssg_conv_desc* d, const float* x, int ldx, float* gamma, int ldg, void* stream);
int ssg_spade_modulate_fwd_f32(const float* x, int ldx, const float* gb, int ldgb, int64_t P, int C, float* y, int ldy, void* stream);
int ssg_spade_modulate_bwd_f32(const float* x, int ldx, const float* gb, int ldgb, const float* dy, int lddy, int64_t P, int C,
                               float* dx, int lddx, float* dgb, int lddgb, void* stream);
/* the same pass that also returns the bias gradients of the gamma / beta convs (normalization.py:94-96):
 * sums[0:C] = sum_p dy*x, sums[C:2C] = sum_p dy, fp64, deterministic; ws: ssg_bn_workspace_bytes(P, C) bytes.  Only the gamma
 * half of `gb` is read (ldgb >= C: a gamma-only tensor from ssg_spade_conv_modulate_f32 is fine). */
int ssg_spade_modulate_bwd_sums_f32(const float* x, int ldx, const float* gb, int ldgb, const float* dy, int lddy, int64_t P,
                                    int C, float* dx, int lddx, float* dgb, int lddgb, double* sums, void* ws, void* stream);
/* The lean SPADE backward: d(beta) = dy is never copied and dx = dy*(1+gamma) is never stored.
 * ssg_spade_modulate_dgamma_sums_f32 reads x and dy only and writes dgamma = dy*x (C channels, pixel stride lddg) and the
 * same 2C fp64 sums in the same layout, bit for bit (same products, same reduction tree, same ordered finalise);
 * ws: ssg_bn_workspace_bytes(P, C) bytes.  16-byte aligned tensors, pixel strides multiples of 4. */
int ssg_spade_modulate_dgamma_sums_f32(const float* x, int ldx, const float* dy, int lddy, int64_t P, int C,
                                       float* dgamma, int lddg, double* sums, void* ws, void* stream);
/* ssg_spade_dgrad_modulate_f32 is the launch ssg_conv2d_f32(d) makes for `d` (no residual, no bias, no activation: the input
 * gradient of SPADE's x2map conv) whose epilogue adds dout[p][c] * (1 + gamma[p][c]) where a residual launch adds res[p][c]:
 *   out = conv + fl(dout * fl(1 + gamma))  -- the same two operations ssg_spade_modulate_bwd_sums_f32 used for its dx, each
 * rounded to fp32, then the residual launch's add (no fused multiply-add): the bits of the pair it replaces.
 * dout / gamma: C = d->Cout channels, 16-byte
 * aligned, pixel strides multiples of 4, under 2^30 elements.  ssg_spade_dgrad_modulate_ok(d): 1 where the launch of `d` runs
 * on a kernel that has this epilogue (the thin-Cin kernels thin32_cin / thin4_cin: 4-channel input, Cout > 8, Cout % 4 == 0),
 * else the caller keeps ssg_spade_modulate_bwd_sums_f32 and a residual launch. */
int ssg_spade_dgrad_modulate_ok(const ssg_conv_desc* d);
int ssg_spade_dgrad_modulate_f32(const ssg_conv_desc* d, const float* dout, int lddout, const float* gamma, int ldg, void* stream);
/* activation backward: dx = dy * (y > 0 ? 1 : slope) (+ add) */
int ssg_act_bwd_f32(const float* y, int ldy, const float* dy, int lddy, int64_t P, int C, int act, float slope, float* dx, int lddx, void* stream);
/* dst[p, 0:C] = src[p, 0:C]: channel-slice copy (materialised torch.cat of > 2 tensors, archs.py:910-925) */
int ssg_copy_channels_f32(const float* src, int ldsrc, int64_t P, int C, float* dst, int lddst, void* stream);
/* out = a + b (gradient accumulation across consumers) */
int ssg_add_f32(const float* a, const float* b, int64_t n, float* out, void* stream);
/* x[isnan(x)] = 0 in place, mask[i] = 1 where it was NaN (train_seg_gan.py:190) */
int ssg_nan_to_zero_f32(float* x, int64_t n, uint8_t* mask, void* stream);
/* out[i] = mask[i] ? 0 : g[i] (gradient of the masking above; out may alias g) */
int ssg_mask_zero_f32(const float* g, const uint8_t* mask, int64_t n, float* out, void* stream);

/* ------------------------------------------------------------------ fused segmentation loss
 * One pass over logits x and target t (both NHWC-with-stride, C channels, S = H*W pixels per
 * sample) produces everything train_seg_gan.py:191-198 needs:
 *   res[0] = BCEDiceLoss (losses.py:274-302)        res[1] = MSELoss (train_seg_gan.py:195)
 *   res[2] = StableBCE mean (losses.py:130-136)     res[3] = 1 - mean_n dice_n
 *   res[4] = iou_score on channels [mc0,C) (metrics.py:6-22)   res[5] = dice_coef (metrics.py:25-35)
 *   res[6] = bce-is-finite flag
 *   stats[n*3 + {0,1,2}] = per-sample (sum p*t, sum p, sum t)  (kept for backward)
 *   stats[3N + {0..4}]   = (|pred&tgt|, |pred|tgt|, sum p*t, sum p, sum t) on channels >= mc0
 *                          (metric partial sums, all-reduced across ranks); stats holds 3N+5 doubles
 * backward: dx = g_seg * dBCEDice/dx + g_mse * dMSE/dx + g_bce * dStableBCE/dx, g_* read from device scalars
 * (NULL = 0); res[3..7] carry no gradient. */
int64_t ssg_seg_loss_workspace_bytes(int N, int64_t S, int C);
int ssg_seg_loss_fwd_f32(const float* x, int ldx, const float* t, int ldt, int N, int64_t S, int C, int mc0,
                         float* res, double* stats, void* ws, void* stream);
int ssg_seg_loss_bwd_f32(const float* x, int ldx, const float* t, int ldt, int N, int64_t S, int C,
                         const float* res, const double* stats, const float* g_seg, const float* g_mse,
                         const float* g_bce, float* dx, int lddx, void* stream);
/* BCEWithLogitsLoss(mean) of n logits x[i*ldx] against a constant label
 * (train_seg_gan.py:204,221-222); backward writes dx[i*lddx] and zeros the pad columns. */
int ssg_bce_logits_const_fwd_f32(const float* x, int n, int ldx, float label, float* loss, void* stream);
int ssg_bce_logits_const_bwd_f32(const float* x, int n, int ldx, float label, const float* g, float* dx, int lddx, void* stream);

/* ------------------------------------------------------------------ optimizer
 * clip_gradient (srgan_utils.py:186-195: elementwise clamp to [-clip, clip]) fused with the
 * torch.optim.Adam update (train_seg_gan.py:212-215,230-233) over a list of tensors.
 * ptrs: device array of 4*ntensors pointers {param, grad, exp_avg, exp_avg_sq}; sizes and
 * block_map as produced by the host helper in ssunet-gan_amd/optim.py.  clip <= 0 = off. */
int ssg_clamp_adam_multi_f32(const void* const* ptrs, const int64_t* sizes, const int32_t* blk_tensor,
                             const int32_t* blk_chunk, int nblocks, float clip, double lr, double beta1,
                             double beta2, double eps, double weight_decay, double bias_corr1,
                             double bias_corr2_sqrt, void* stream);
/* The same clamp fused with the torch.optim.SGD update, the other optimizer the stage-1 config offers
 * (scripts/train.py:292-294: momentum, nesterov, weight_decay).  Same plan; the record is
 * {param, grad, momentum_buffer, flags}: flags bit 0 set = first momentum step of this tensor (the
 * buffer is written with the gradient and not read), momentum_buffer null when momentum == 0.
 *   g = clamp(grad); grad = g (clip > 0); g += weight_decay * p;
 *   buf = first ? g : momentum * buf + (1 - dampening) * g; g = nesterov ? g + momentum * buf : buf;
 *   p -= lr * g */
int ssg_clamp_sgd_multi_f32(const void* const* ptrs, const int64_t* sizes, const int32_t* blk_tensor,
                            const int32_t* blk_chunk, int nblocks, float clip, double lr, double momentum,
                            double dampening, double weight_decay, int nesterov, void* stream);
int ssg_clamp_f32(float* x, int64_t n, float lo, float hi, void* stream);
/* clamp member `which` (0 param, 1 grad, 2 exp_avg, 3 exp_avg_sq) of every record of `ptrs` in one
 * launch -- stage 1 clamps the WEIGHTS to +-clip every step (train.py:111-112) */
int ssg_clamp_multi_f32(const void* const* ptrs, const int64_t* sizes, const int32_t* blk_tensor, const int32_t* blk_chunk,
                        int nblocks, int which, float lo, float hi, void* stream);

/* per-channel sums over pixels: out[c] = sum_p x[p,c] (bias gradients) */
int ssg_channel_sum_f32(const float* x, int64_t P, int C, int ld, float* out, void* ws, void* stream);

/* ------------------------------------------------------------------ unwired per-op kernels
 * Depthwise convolution (groups = C): EfficientNet MBConv k in {3,5}, s in {1,2} with TF "same"
 * static padding (efficientnet_pytorch/model.py:46-50, utils.py:123-146) and the 9x9 gate conv of
 * xresidualblock.py:16.  `w` is the reference's [C][1][KH][KW] parameter tensor as is.
 *   fwd  : out[n,oy,ox,c] = bias[c] + sum_k in[n, oy*s+ky-pad_top, ox*s+kx-pad_left, c] * w[c,ky,kx]
 *   dgrad: gradient w.r.t. in;  wgrad: gradient w.r.t. w (fp64 two-stage reduction, deterministic) */
int ssg_dwconv2d_fwd_f32(const float* in, int N, int H, int W, int C, int ld, const float* w, const float* bias, int KH, int KW,
                         int stride, int pad_top, int pad_left, int OH, int OW, float* out, int ldo, void* stream);
int ssg_dwconv2d_dgrad_f32(const float* dout, int lddo, int N, int H, int W, int C, const float* w, int KH, int KW, int stride,
                           int pad_top, int pad_left, int OH, int OW, float* dx, int lddx, void* stream);
int64_t ssg_dwconv2d_wgrad_workspace_bytes(int N, int OH, int OW, int C, int KH, int KW);
/* ssg_dwconv2d_kernel_id: the kernel the three entry points above launch (the function they themselves switch on; test and
 * profiling labels).  op: 0 = fwd, 1 = dgrad, 2 = wgrad; pad_left as passed to the entry point; NDH = N * rows of the tensor
 * the call writes (N*OH for fwd, N*H for dgrad; unused by wgrad); aligned16 = both tensor pointers are 16-byte aligned
 * (unused by wgrad).  Returns -1 for another op, else
 *   fwd  :  0 = dw_fwd_kernel (generic),  1 = dw_s1_kernel<KW,T,1> (stride 1, KW in {3,5,7,9}),
 *           2 = dw_s1_kernel<KW,T,2> (stride 2, KH == KW in {3,5});
 *   dgrad: 10 = dw_dgrad_kernel (generic), 11 = dw_s1_kernel<KW,T,1> on the flipped kernel with pads K-1-pad,
 *          12 / 13 = dw_dgrad_s2_kernel<KW,T,PLODD = 0 / 1> (pad_left even / odd);
 *   wgrad: 20 = dw_wgrad_partial_kernel (generic), 21 / 22 = dw_wgrad_s1_kernel<KW,T,S = 1 / 2>;
 * the tiled fwd / dgrad kernels need aligned16, NDH <= 65535 and (C/4 + 15)/16 <= 65535 (grid.y / grid.z). */
int ssg_dwconv2d_kernel_id(int op, int stride, int KH, int KW, int pad_left, int64_t NDH, int C, int aligned16);
int ssg_dwconv2d_wgrad_f32(const float* in, int N, int H, int W, int C, int ld, const float* dout, int lddo, int KH, int KW,
                           int stride, int pad_top, int pad_left, int OH, int OW, float* dw, void* ws, void* stream);
/* element-wise: swish x*sigmoid(x) with the reference's backward (efficientnet_pytorch/utils.py:37-48),
 * sigmoid (SE gate, model.py:79), Gaussian exp(-x^2) (xresidualblock.py:5-7).  The forward takes the REAL channel count C (any
 * C > 0, pixel strides multiples of 4) and writes the pad lanes [C, pad4(C)) as 0: sigmoid(0) and exp(-0) are not. */
#define SSG_UNARY_SWISH 0
#define SSG_UNARY_SIGMOID 1
#define SSG_UNARY_GAUSSIAN 2
int ssg_unary_fwd_f32(const float* x, int ldx, int64_t P, int C, int op, float* y, int ldy, void* stream);
int ssg_unary_bwd_f32(const float* x, int ldx, const float* dy, int lddy, int64_t P, int C, int op, float* dx, int lddx, void* stream);
/* y = a*b (xresidualblock.py:23) and its gradients */
int ssg_mul_fwd_f32(const float* a, int lda, const float* b, int ldb, int64_t P, int C, float* y, int ldy, void* stream);
int ssg_mul_bwd_f32(const float* a, int lda, const float* b, int ldb, const float* dy, int lddy, int64_t P, int C,
                    float* da, int ldda, float* db, int lddb, void* stream);
/* squeeze-excite plumbing (model.py:76-80): y[n,p,c] = x[n,p,c]*s[n,c]; out[n,c] = scale*sum_p a[n,p,c]*(b?b[n,p,c]:1)
 * (global average pool and the gate's gradient); y[n,p,c] = scale*s[n,c] (average-pool backward) */
int ssg_channel_scale_fwd_f32(const float* x, int ldx, const float* s, int N, int64_t S, int C, float* y, int ldy, void* stream);
int64_t ssg_sample_channel_sum_workspace_bytes(int N, int64_t S, int C);
int ssg_sample_channel_sum_f32(const float* a, int lda, const float* b, int ldb, int N, int64_t S, int C, float scale, float* out,
                               void* ws, void* stream);
int ssg_broadcast_rows_f32(const float* s, int N, int64_t S, int C, float scale, float* y, int ldy, void* stream);
/* Spectral norm (spectral_norm.py:38-88): power iteration on W [rows][cols] with in-place u [rows],
 * v [cols]; W_out = W / sigma (W_out may be NULL: sigma only), sigma = u.(W v).  Backward treats u, v as constants:
 * dW = dWsn/sigma - (sum(dWsn.W)/sigma^2) u v^T. */
int64_t ssg_spectral_norm_workspace_bytes(int rows, int cols);
int ssg_spectral_norm_fwd_f32(const float* W, int rows, int cols, float* u, float* v, int n_power_iterations, double eps,
                              float* W_out, float* sigma, void* ws, void* stream);
int ssg_spectral_norm_bwd_f32(const float* dWsn, const float* W, int rows, int cols, const float* u, const float* v,
                              const float* sigma, float* dW, void* ws, void* stream);

/* ------------------------------------------------------------------ squeeze-excite gate (se_gate.hip)
 * efficientnet_pytorch/model.py:83-87: x_squeezed = adaptive_avg_pool2d(x, 1); _se_expand(swish(_se_reduce(x_squeezed)));
 * x = sigmoid(x_squeezed) * x.  These entry points replace the two 1x1 convs on the pooled [N][C] vector, the swish between
 * them and the sigmoid after them (the pooling and the gating product stay ssg_sample_channel_sum_* / ssg_channel_scale_*):
 *   h_pre[n][s] = b1[s] + sum_c w1[s][c] * sq[n][c]          (w1 = _se_reduce.weight [S][C][1][1], b1 may be NULL)
 *   gate[n][c]  = sigmoid(b2[c] + sum_s w2[c][s] * swish(h_pre[n][s]))   (w2 = _se_expand.weight [C][S][1][1])
 * h_pre ([N][S], dense) is kept for the backward.  Range: N <= 16, S <= 256, N*S <= 2048 (ssg_se_gate_ok; outside it the
 * caller keeps the conv path).  Backward: from dgate it writes dsq [N][C] (stride lds_), dw1 [S][C], db1 [S] (may be NULL),
 * dw2 [C][S], db2 [C] (may be NULL).  tmp = ssg_se_gate_workspace_floats(N, C, S) floats of scratch in either direction
 * (partial sums per 64-channel chunk; dz in the backward; the entry points cannot check its size).  All sums run in a fixed
 * order.  Alignment: when S % 4 == 0 the rows of w2 (and dw2 in the backward) are accessed 16 bytes at a time, so w2 / dw2 must
 * be 16-byte aligned (SSG_EALIGN otherwise) -- a view at an odd offset inside a flat parameter buffer is refused, not mis-read. */
int ssg_se_gate_ok(int N, int C, int S);
int64_t ssg_se_gate_workspace_floats(int N, int C, int S);
int ssg_se_gate_fwd_f32(const float* sq, int ldq, int N, int C, const float* w1, const float* b1, const float* w2, const float* b2,
                        int S, float* h_pre, float* gate, int ldg, float* tmp, void* stream);
int ssg_se_gate_bwd_f32(const float* dgate, int ldd, const float* gate, int ldg, const float* h_pre, const float* sq, int ldq, int N, int C,
                        const float* w1, const float* w2, int S, float* dsq, int lds_, float* dw1, float* db1, float* dw2, float* db2,
                        float* tmp, void* stream);

/* ------------------------------------------------------------------ calibration (bench only)
 * Measured ceilings of the device the job runs on: back-to-back fp32 32x32x2 MFMA issue
 * (FLOPs = blocks*4*iters*16*4096; scratch holds blocks*256 floats) and a 16-B/lane HBM copy. */
int ssg_tool_mfma_peak_f32(float* scratch, int blocks, int iters, void* stream);
/* the same loop with v_mfma_f32_32x32x16_bf16 (32768 FLOP each): the ceiling of the split-operand kernels on this device */
int ssg_tool_mfma_peak_bf16(float* scratch, int blocks, int iters, void* stream);
/* ... on caller operands (`data`: 64 KiB of bf16 values), which toggle the multiplier inputs: the power-limited rate */
int ssg_tool_mfma_peak_bf16_data(float* scratch, int blocks, int iters, const void* data, void* stream);
int ssg_tool_mfma_peak_bf16_data16(float* scratch, int blocks, int iters, const void* data, void* stream);   /* the same on v_mfma_f32_16x16x32_bf16 */
int ssg_tool_copy_f32(const float* src, float* dst, int64_t n, void* stream);   /* one float4 per thread, non-temporal */

/* ------------------------------------------------------------------ sliding-window inference (HBM-bound)
 * The two host loops around the generator forward of aerial_image_segmentation_api.py, restated bit for bit.
 * Origins: P pairs (h1, w1) of int32, top-left corners of p_size x p_size patches.  `org` is the DEVICE array the kernels
 * read; `org_host` is the caller's HOST copy of the same values, which the entry point checks (every patch inside the
 * H x W image) before it launches -- a patch outside the image is refused with SSG_EINVAL and nothing is enqueued.
 *
 * ssg_sw_gather_patches_u8_f32 (get_patched_input, api.py:336-373): img is [H][W][3] uint8 (BGR, 4-byte aligned); out is
 * [P, 3, out_size, out_size] fp32 NHWC with ld = 4, pad lane written as 0.  p_size / out_size is 1 (the byte itself) or 2
 * ((a + b + c + d + 2) >> 2 of the 2x2 box); then ((float)v - mean[c]) * rdenom[c], then / 255.0f, each one fp32 rounding.
 * mean / rdenom are albumentations Normalize()'s fp32 mean * 255 and 1 / (std * 255), computed by the caller.
 *
 * ssg_sw_merge_masks_f32_u8 (patch_merge, api.py:119-217): probs is [P, C, S, S] fp32 NHWC with pixel stride ld,
 * p_size / S is 1 or 2, weight[p] (int32, >= 0) is the number of times patch p counts; out is [C][H][W] uint8 in {0, 255}.
 * Per pixel and class, over the patches that cover it: u8 = (uint8)(p * 255.0f), resized to p_size (2x: 0.25 / 0.75 taps,
 * edge-clamped, rounded half up), counted if > 127; k = sum of the weights that counted, n = sum of the weights (0 -> 1);
 * out = (int)((double)k / n * 255.0) > 127 ? 255 : 0.  One thread per pixel, no atomics: deterministic. */
int ssg_sw_gather_patches_u8_f32(const uint8_t* img, int H, int W, const int32_t* org, const int32_t* org_host, int P,
                                 int p_size, int out_size, float mean0, float mean1, float mean2,
                                 float rdenom0, float rdenom1, float rdenom2, float* out, void* stream);
int ssg_sw_merge_masks_f32_u8(const float* probs, int ld, int P, int C, int S, const int32_t* org, const int32_t* org_host,
                              const int32_t* weight, int p_size, int H, int W, uint8_t* out, void* stream);

/* The ground-truth branch of the same pipeline (mask_convert and the evaluation of the two mask sets,
 * aerial_image_segmentation_api.py:220-236,394-406): every value is an integer, so both are exact.
 *
 * ssg_sw_gather_labels_u8_f32 (api.py:220-236,394-406): label is [H][W][3] uint8 (BGR label image, 4-byte aligned), origins as
 * above; out is [P, C, out_size, out_size] fp32 NHWC with ld = 4, 1 <= C <= 3, holding 0.0f or 1.0f -- mask_convert(patch, c,
 * out_size) / 255.0 for c < C -- and +0.0f in the lanes C .. 3.  A pixel selects class 0 / 1 / 2 when its three bytes, in memory
 * order, are (255, 255, 255) / (255, 0, 0) / (0, 0, 255).  p_size / out_size = 1: the selection itself; = 2: at least 2 of the
 * 2 x 2 box selected (resize_u8 at 1/2 gives (255 k + 2) >> 2 in {0, 64, 128, 191, 255}; post_process_resized_mask sends 64 to
 * 0 and 128, 191 to 255).
 *
 * ssg_sw_mask_counts_u8 (api.py:394-406, the two mask lists it returns): pred and gt are [C][HW] uint8 (any alignment);
 * counts is uint64 [C][3] on the device, 8-byte aligned, zeroed by the caller before the first call: the entry ADDS, per class,
 * the number of pixels with pred > 127 and gt > 127, with pred > 127, and with gt > 127.  Integer sums combined with 64-bit
 * integer atomics: exact and independent of the order. */
int ssg_sw_gather_labels_u8_f32(const uint8_t* label, int H, int W, const int32_t* org, const int32_t* org_host, int P,
                                int p_size, int out_size, int C, float* out, void* stream);
int ssg_sw_mask_counts_u8(const uint8_t* pred, const uint8_t* gt, int C, int64_t HW, uint64_t* counts, void* stream);

/* Flip / rotation test-time augmentation around the same pipeline.  A view is a D4 code k in 0 .. 7 with
 * f = k >> 2, r = k & 3: T_k(a) = rot90(fliplr(a) if f else a, r) on a square [S, S] array, rot90 counter-clockwise
 * (rot90(a)[i, j] = a[j, S - 1 - i]); T_k^-1(y) = fliplr(u) if f else u with u = rot90(y, 4 - r).  Moves and exact scalings only:
 * both entries are bit for bit what the definitions say.
 *
 * ssg_sw_gather_patches_d4_u8_f32: ssg_sw_gather_patches_u8_f32 with `orient`, one code per launch: pixel (i, j) of patch p is
 * pixel (i, j) of T_orient of the patch that entry writes (orient 0: the same values).  Same layout ([P, 3, out_size, out_size]
 * NHWC, ld 4, pad lane 0), rounding steps, mean / rdenom and org / org_host contract; orient outside 0 .. 7 is refused with
 * SSG_EINVAL and nothing is enqueued.
 *
 * ssg_sw_tta_reduce_f32: src holds K views of [B, C, S, S] fp32 NHWC probabilities with pixel stride ld, view k starting
 * `slab` floats after view k - 1 (slab >= B * S * S * ld, a multiple of 4); codes is a HOST array of K ints, read before the launch
 * and never on the device.  out[b, c] = tree-mean over k of T_codes[k]^-1(src[k, b, c]) for c < C, into a [B, C, S, S] NHWC tensor
 * (or batch slice) with pixel stride ldo; every lane C .. ldo - 1 of out gets +0.0f, and no lane C .. ld - 1 of src reaches a
 * result.  The mean is a balanced tree in list order in fp32 -- K = 8: (((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7))) * (1 / K),
 * K = 4: ((q0 + q1) + (q2 + q3)) * (1 / K), K = 2: (q0 + q1) * (1 / K), K = 1: q0 -- so K equal views give back that view.
 * Refused with SSG_EINVAL before any launch: K not in {1, 2, 4, 8}, a code outside 0 .. 7, a repeated code, C > ld or ldo,
 * B, C or S <= 0.  out must not overlap src.  One writer per element, no atomics: deterministic. */
int ssg_sw_gather_patches_d4_u8_f32(const uint8_t* img, int H, int W, const int32_t* org, const int32_t* org_host, int P,
                                    int p_size, int out_size, int orient, float mean0, float mean1, float mean2,
                                    float rdenom0, float rdenom1, float rdenom2, float* out, void* stream);
int ssg_sw_tta_reduce_f32(const float* src, int64_t slab, int ld, int K, const int32_t* codes, int B, int C, int S,
                          float* out, int ldo, void* stream);

/* Confidence maps of the same pipeline.  With r_j the resized uint8 value of covering patch j at a pixel (as in
 * ssg_sw_merge_masks_f32_u8: (uint8)(p * 255.0f), at 2x (9a + 3b + 3c + d + 8) >> 4 over the edge-clamped taps), m_j its weight
 * and n their sum (0 -> 1), on(t) = (int)((double)(sum of m_j with r_j > t) / n * 255.0) > 127 for t in 0 .. 254 -- the mask
 * patch_merge gives with its first-stage level at t instead of 127 -- and the score S = #{t : on(t)} in 0 .. 255.  on(t) is
 * non-increasing in t, so on(t) <=> S > t, and S > 127 is the mask of ssg_sw_merge_masks_f32_u8 bit for bit.
 *
 * ssg_sw_merge_scores_f32_u8: probs, ld, P, C, S, org, org_host, weight, p_size, H, W as ssg_sw_merge_masks_f32_u8; out is
 * [C][H][W] uint8.  thr_host == NULL: out = S.  Otherwise thr_host is a HOST array of C int32 levels in 0 .. 254 (C <= 64), read
 * before the launch and never on the device: out[c] = S[c] > thr_host[c] ? 255 : 0, in one walk over the patches like the mask
 * entry.  Score mode finds S by an 8-step bisection, one walk per step; exact for any number of covering patches.  Refused
 * with SSG_EINVAL before any launch: a null pointer (thr_host excepted), P <= 0, a factor other than 1 and 2, a patch outside
 * the image, a level outside 0 .. 254.  One thread per pixel, no atomics: deterministic.
 *
 * ssg_sw_score_hist_u8: scores and gt are [C][HW] uint8 (any alignment); hist is int64 [C][2][256] on the device, 8-byte aligned,
 * zeroed by the caller before the first call: the entry ADDS, per class c and pixel, one to hist[c][gt > 127][score].  64-bit
 * integer atomics: exact and independent of the order.  The counts of every level t follow as suffix sums over score > t. */
int ssg_sw_merge_scores_f32_u8(const float* probs, int ld, int P, int C, int S, const int32_t* org, const int32_t* org_host,
                               const int32_t* weight, int p_size, int H, int W, const int32_t* thr_host, uint8_t* out, void* stream);
int ssg_sw_score_hist_u8(const uint8_t* scores, const uint8_t* gt, int C, int64_t HW, int64_t* hist, void* stream);

/* ------------------------------------------------------------------ training augmentation (HBM-bound)
 * ssg_augment_batch_u8_f32: one launch turns a batch of uint8 source tiles into the network's input and target.  img is
 * [N][H][W][3] uint8 (B, G, R), mask [N][H][W][C] uint8, C in 1 .. 8, any alignment.  params is the DEVICE table the kernel
 * reads, int32 [N][16]; params_host the caller's HOST copy of the same values, which the entry point checks before it launches;
 * lut is uint8 [N][256] on the device.  A row holds m0 .. m5, flags, dh, ds, dv and six zeros.
 *   Geometry: m0 .. m5 are 16.16 fixed point; output pixel (i, j) (row, column) reads the source at sx = m0 j + m1 i + m2,
 *   sy = m3 j + m4 i + m5 in int64 (pixel-index coordinates: the half-pixel shifts are folded into m2 and m5).  Image: bilinear,
 *   x0 = sx >> 16, fx = (sx >> 8) & 255, likewise y; the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) weigh
 *   (256 - fx)(256 - fy), fx (256 - fy), (256 - fx) fy, fx fy; a tap outside the source is the byte border[c] and is never read;
 *   v = (sum + 2^15) >> 16.  Mask: nearest, (sx + 2^15) >> 16 and (sy + 2^15) >> 16, 0 outside.
 *   Colour: if flags bit 0 is set, (B, G, R) -> integer H in 0 .. 179, S, V in 0 .. 255 (round-half-up divisions),
 *   H = (H + dh) mod 180, S = clip(S + ds), V = clip(V + dv), and back in integers; then every byte indexes the sample's lut.
 *   Output: out_img is [N, 3, out_h, out_w] fp32 NHWC with ld = 4, ((float)byte - mean[c]) * rdenom[c] (two fp32 roundings;
 *   mean / rdenom as in ssg_sw_gather_patches_u8_f32, no further / 255), pad lane 0; out_tgt is [N, C, out_h, out_w] fp32 NHWC
 *   with ld = C rounded up to 4, (float)mask byte, pad lanes 0.  Both 16-byte aligned.
 * tests/augment_ref.py states all of it in numpy; the entry is that bit for bit.  Refused with SSG_EINVAL before any launch:
 * a null pointer, N, H, W, out_h or out_w <= 0, C outside 1 .. 8, a border value outside 0 .. 255, a params_host row with a flag
 * bit other than bit 0, |dh| > 179, |ds| or |dv| > 255, or a map whose coordinates would leave int64.  One writer per element. */
int ssg_augment_batch_u8_f32(const uint8_t* img, const uint8_t* mask, int N, int H, int W, int C, const int32_t* params,
                             const int32_t* params_host, const uint8_t* lut, int out_h, int out_w,
                             int border0, int border1, int border2, float mean0, float mean1, float mean2,
                             float rdenom0, float rdenom1, float rdenom2, float* out_img, float* out_tgt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
