// Implicit-GEMM convolution for gfx950 (MI355X): fp32 in, fp32 accumulate on
// v_mfma_f32_32x32x2_f32.  ABI + semantics: include/ssunet_hip.h (ssg_conv2d_igemm_f32).
//
// GEMM view: M = pixels of a (TH x 16) spatial patch of one image, N = output channels,
// K = taps x input channels, walked 16 channels ("a K-step") at a time.
//   - A tile [BM pixels][16 ch] is gathered from NHWC global memory: each lane fetches one
//     16-byte channel quad of one pixel (64 B of contiguous channels per pixel per K-step,
//     so a wave's loads cover whole 64-B segments); out-of-image taps are predicated to 0.
//   - B tile [BN couts][16 k] comes from the pre-packed [Cout][Kp] weight matrix: rows are
//     K-contiguous, so B loads are the same 16-byte-quad pattern.
//   - both tiles sit in LDS as [row][16 + 4 pad] floats (80-B rows): ds_read_b128 of one
//     row-per-lane is bank-conflict free (5*row mod 16 distinct within every 16-lane group).
//   - MFMA operand trick: one ds_read_b128 gives a lane 4 consecutive channels; lanes 0-31
//     read channels [8h, 8h+4), lanes 32-63 read [8h+4, 8h+8), so register j of the read is
//     the (k=0 | k=1) operand pair (8h+j | 8h+4+j) of one 32x32x2 MFMA.  A and B use the same
//     pairing, so 2+2 reads feed 4x(MI*NI) MFMAs.
//   - register-staged double buffer: global loads for step s+1 are issued before the MFMAs
//     of step s and written to the other LDS buffer after them; one barrier per K-step.
//     Each K-step is MI*NI*8 MFMAs x 64 cycles per wave, long enough to cover L2/HBM latency.
#include "common.h"
#include "conv_thin.h"
#include "conv_args.h"

namespace {

constexpr int LDS_ROW = 20;   // floats per LDS row (16 data + 4 pad = 80 bytes)

template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const ConvArgs a) {
  static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
  constexpr int TH = BM / 16;
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int MI = WTM / 32, NI = WTN / 32;
  constexpr int A_LD = BM * 4 / 256;                   // float4 loads per thread for A
  constexpr int B_LD = (BN * 4 + 255) / 256;           // ... for B
  static_assert(MI >= 1 && NI >= 1, "wave tile");

  __shared__ __attribute__((aligned(16))) float lds[2 * (BM + BN) * LDS_ROW];
  float* As = lds;
  float* Bs = lds + 2 * BM * LDS_ROW;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;

  // ---- tile decode
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x; bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int n = bid / a.tiles_y;
  const int n0 = blockIdx.y * BN;
  const int Cin = a.C1 + a.C2;

  // ---- per-thread A gather coordinates (fixed over the K loop)
  int a_iy0[A_LD], a_ix0[A_LD];
  bool a_ok[A_LD];
  const int q = tid & 3;
#pragma unroll
  for (int j = 0; j < A_LD; ++j) {
    const int p = (tid >> 2) + 64 * j;
    const int gy = ty * TH + (p >> 4), gx = tx * 16 + (p & 15);
    a_ok[j] = (gy < a.GH) && (gx < a.GW);
    a_iy0[j] = gy * a.in_sy;
    a_ix0[j] = gx * a.in_sx;
  }
  // ---- per-thread B rows
  const float* b_ptr[B_LD];
  bool b_ok[B_LD];
#pragma unroll
  for (int j = 0; j < B_LD; ++j) {
    const int r = (tid >> 2) + 64 * j;
    b_ok[j] = (r < BN) && (n0 + r < a.Cout);
    b_ptr[j] = a.w + (size_t)(n0 + (b_ok[j] ? r : 0)) * a.Kp + 4 * q;
  }

  f32x4 ra[A_LD], rb[B_LD];

  auto load_step = [&](int s) {
    int t, c;
    if (a.kmode == 0) {
      const int chunk = s / a.ntaps;
      t = s - chunk * a.ntaps;
      c = chunk * 16 + 4 * q;
    } else {
      const int k = s * 16 + 4 * q;
      t = k / Cin;
      c = k - t * Cin;
    }
    const bool tv = t < a.ntaps;
    const int dy = ssg_tap_dy(a.tap_bits, tv ? t : 0), dx = ssg_tap_dx(a.tap_bits, tv ? t : 0);
    const float* src; int ld, cc;
    if (c < a.C1) { src = a.in1; ld = a.ld1; cc = c; }
    else          { src = a.in2; ld = a.ld2; cc = c - a.C1; }
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      const int iy = a_iy0[j] + dy, ix = a_ix0[j] + dx;
      const bool ok = tv && a_ok[j] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (ok) v = *(const f32x4*)(src + ((size_t)(n * a.H + iy) * a.W + ix) * ld + cc);
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (b_ok[j]) v = *(const f32x4*)(b_ptr[j] + (size_t)s * 16);
      rb[j] = v;
    }
  };
  auto store_step = [&](int buf) {
    float* Ab = As + buf * BM * LDS_ROW;
    float* Bb = Bs + buf * BN * LDS_ROW;
#pragma unroll
    for (int j = 0; j < A_LD; ++j)
      *(f32x4*)(Ab + ((tid >> 2) + 64 * j) * LDS_ROW + 4 * q) = ra[j];
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
      const int r = (tid >> 2) + 64 * j;
      if (r < BN) *(f32x4*)(Bb + r * LDS_ROW + 4 * q) = rb[j];
    }
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  load_step(0);
  store_step(0);
  __syncthreads();

  const int half = lane >> 5, l31 = lane & 31;
  for (int s = 0; s < a.nsteps; ++s) {
    const int buf = s & 1;
    const bool more = (s + 1) < a.nsteps;
    if (more) load_step(s + 1);
    const float* Ab = As + buf * BM * LDS_ROW + (wm * WTM + l31) * LDS_ROW + 4 * half;
    const float* Bb = Bs + buf * BN * LDS_ROW + (wn * WTN + l31) * LDS_ROW + 4 * half;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 fa[MI], fb[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = *(const f32x4*)(Ab + i * 32 * LDS_ROW + 8 * h);
#pragma unroll
      for (int j = 0; j < NI; ++j) fb[j] = *(const f32x4*)(Bb + j * 32 * LDS_ROW + 8 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
    }
    if (more) store_step(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: C/D map of 32x32 tiles: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int co = n0 + wn * WTN + j * 32 + l31;
    const bool cok = co < a.Cout;
    const float bv = (a.bias && cok) ? a.bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const int gy = ty * TH + (p >> 4), gx = tx * 16 + (p & 15);
        if (gy < a.GH && gx < a.GW) {
          const size_t pix = ((size_t)(n * a.OH + gy * a.out_sy + a.out_oy) * a.OW + gx * a.out_sx + a.out_ox);
          float v = acc[i][j][r] + bv;
          if (cok) {
            if (a.res) v += a.res[pix * a.ldr + co];
            if (a.act == SSG_ACT_RELU) v = v < 0.f ? 0.f : v;
            else if (a.act == SSG_ACT_LRELU) v = v > 0.f ? v : v * a.slope;
            a.out[pix * a.ldo + co] = v;
          } else if (co < ((a.Cout + 3) & ~3)) {
            a.out[pix * a.ldo + co] = 0.f;      // keep pad channels finite (zero)
          }
        }
      }
    }
  }
}

template <int BM, int BN, int WAVES_M, int WAVES_N>
int launch(const ConvArgs& a0, hipStream_t st) {
  ConvArgs a = a0;
  constexpr int TH = BM / 16;
  a.tiles_x = (a.GW + 15) / 16;
  a.tiles_y = (a.GH + TH - 1) / TH;
  dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.N), (unsigned)((a.Cout + BN - 1) / BN));
  hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WAVES_M, WAVES_N>), grid, dim3(256), 0, st, a);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

// tile choice: wide-N tiles for Cout >= 96, narrow for the 64/32/small-Cout layers.
int pick_variant(const ssg_conv_desc* d) {
  if (d->Cout > 64) return 0;       // 128 x 128
  if (d->Cout > 32) return 1;       // 256 x 64
  return 2;                         // 256 x 32
}

// LDS-DMA pipeline (conv_igemm_dma.hip) for the dense layers; kmode 1 and the narrow outputs below stay on the
// register-staged kernel.
bool uses_halo(const ConvArgs& a);

bool uses_dma(const ssg_conv_desc* d) {
  if (d->kmode != 0) return false;
  if (d->Cout > 32) return true;
  // Cout 17..32 on a small pixel grid with a long reduction (the input gradient of SPADE's gamma|beta conv at the 32x32
  // level: 1024 -> 32 on 16 384 pixels = 64 tiles of the 256x32 register kernel): the 64-wide halo tile multiplies half
  // its columns by zero weights but splits K over the idle CUs (15 -> > 60 TFLOP/s)
  return d->Cout > 16 && d->ntaps == 9 && d->in_sy == 1 && d->in_sx == 1 && d->C1 + d->C2 >= 256 &&
         (long long)d->N * d->GH * d->GW <= 32768 && uses_halo(ssg_conv_to_args(d));
}

// LDS-resident halo tile (conv_igemm_halo.hip) for the 3x3 window
bool uses_halo(const ConvArgs& a) { return ssg_conv_halo_ok(a); }

int validate(const ssg_conv_desc* d) {
  SSG_REQUIRE(d != nullptr, SSG_EINVAL, "conv: null desc");
  SSG_REQUIRE(d->in1 && d->w && d->out, SSG_EINVAL, "conv: null pointer");
  SSG_REQUIRE(d->C1 > 0 && d->C1 % 4 == 0 && d->C2 >= 0 && d->C2 % 4 == 0, SSG_EINVAL,
              "conv: C1=%d C2=%d must be multiples of 4", d->C1, d->C2);
  SSG_REQUIRE(d->C2 == 0 || d->in2, SSG_EINVAL, "conv: C2 > 0 needs in2");
  SSG_REQUIRE(d->ld1 >= d->C1 && d->ld1 % 4 == 0 && (d->C2 == 0 || (d->ld2 >= d->C2 && d->ld2 % 4 == 0)), SSG_EALIGN,
              "conv: input pixel strides");
  SSG_REQUIRE(ssg_aligned16(d->in1) && ssg_aligned16(d->in2) && ssg_aligned16(d->w), SSG_EALIGN, "conv: 16-B alignment");
  SSG_REQUIRE(d->Kp > 0 && d->Kp % 16 == 0, SSG_EINVAL, "conv: Kp=%d", d->Kp);
  SSG_REQUIRE(d->ntaps >= 1 && d->ntaps <= SSG_MAX_TAPS, SSG_EINVAL, "conv: ntaps=%d", d->ntaps);
  const int Cin = d->C1 + d->C2;
  if (d->kmode == 0) {
    SSG_REQUIRE(Cin % 16 == 0 && d->C1 % 16 == 0, SSG_EINVAL, "conv: kmode 0 needs 16-channel multiples (C1=%d C2=%d)", d->C1, d->C2);
    SSG_REQUIRE(d->Kp == Cin * d->ntaps, SSG_EINVAL, "conv: Kp=%d != Cin*ntaps=%d", d->Kp, Cin * d->ntaps);
  } else {
    SSG_REQUIRE(d->kmode == 1, SSG_EINVAL, "conv: kmode=%d", d->kmode);
    SSG_REQUIRE(d->Kp >= Cin * d->ntaps && d->Kp < Cin * d->ntaps + 16, SSG_EINVAL, "conv: Kp=%d vs K=%d", d->Kp, Cin * d->ntaps);
  }
  SSG_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->GH > 0 && d->GW > 0 && d->Cout > 0, SSG_EINVAL, "conv: empty dims");
  SSG_REQUIRE(d->ldo >= d->Cout, SSG_EINVAL, "conv: ldo=%d < Cout=%d", d->ldo, d->Cout);
  SSG_REQUIRE((d->GH - 1) * d->out_sy + d->out_oy < d->OH && (d->GW - 1) * d->out_sx + d->out_ox < d->OW, SSG_EINVAL,
              "conv: pixel grid exceeds the output image");
  SSG_REQUIRE(d->res == nullptr || d->ldr >= d->Cout, SSG_EINVAL, "conv: residual stride");
  for (int t = 0; t < d->ntaps; ++t)
    SSG_REQUIRE(d->dy[t] >= -2 && d->dy[t] <= 5 && d->dx[t] >= -2 && d->dx[t] <= 5, SSG_EINVAL, "conv: tap offset out of range");
  SSG_REQUIRE((int64_t)d->N * d->H * d->W * (int64_t)(d->ld1 > d->ld2 ? d->ld1 : d->ld2) < (1ll << 40), SSG_EINVAL, "conv: tensor too large");
  return SSG_OK;
}

}  // namespace

// The descriptor as the kernels' argument block (no checks), also for the bf16 launchers (conv_k32_bf16_host.h)
ConvArgs ssg_conv_to_args(const ssg_conv_desc* d) {
  ConvArgs a;
  a.in1 = d->in1; a.in2 = d->C2 ? d->in2 : d->in1; a.w = d->w; a.bias = d->bias; a.res = d->res; a.out = d->out;
  a.bnpart = d->bnpart;
  a.C1 = d->C1; a.C2 = d->C2; a.ld1 = d->ld1; a.ld2 = d->C2 ? d->ld2 : d->ld1;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Kp = d->Kp; a.kmode = d->kmode;
  a.ldr = d->ldr; a.Cout = d->Cout; a.ldo = d->ldo;
  a.GH = d->GH; a.GW = d->GW; a.OH = d->OH; a.OW = d->OW;
  a.in_sy = d->in_sy; a.in_sx = d->in_sx; a.out_sy = d->out_sy; a.out_sx = d->out_sx;
  a.out_oy = d->out_oy; a.out_ox = d->out_ox;
  a.ntaps = d->ntaps;
  a.tap_bits = ssg_pack_taps(d->dy, d->dx, d->ntaps);
  a.act = d->act; a.slope = d->slope;
  a.nsteps = d->Kp / 16;
  a.tiles_x = a.tiles_y = 0;
  a.ws = nullptr; a.ksplit = 1;
  a.parity = d->parity_merge;
  a.w32 = d->w;
  a.in_scale = d->in_scale; a.in_shift = d->in_shift; a.in_act = d->in_act; a.in_slope = d->in_slope;
  a.bwd_x = d->bwd_x; a.bwd_ldx = d->bwd_ldx; a.bwd_scale = d->bwd_scale; a.bwd_shift = d->bwd_shift; a.bwd_mean = d->bwd_mean;
  a.bwd_act = d->bwd_act; a.bwd_slope = d->bwd_slope;
  return a;
}

namespace {

// The kernel families in the order the dispatcher tries them: thin VALU / 4x4x1 kernels and the streaming 1x1 kernel for the
// few-channel shapes, then on the MFMA path the split-operand kernels (bf16 terms on the bf16 matrix pipe; only with w_split) and
// the fp32 kernels (LDS halo tile, LDS-DMA pipeline, register-staged).
enum ConvKind { KIND_THIN4, KIND_THIN, KIND_1X1, KIND_K32, KIND_PARITY, KIND_HALO_X3, KIND_DMA_X3, KIND_HALO, KIND_DMA, KIND_REG };

struct ConvPlan {
  int rc;            // validate(d); nothing below is set unless SSG_OK
  ConvArgs a;        // kernel arguments of the descriptor as given (split-K and w_split applied by the launch)
  ConvKind kind;
  int variant;       // KIND_THIN4 / THIN: the thin kind; fp32 MFMA kinds: pick_variant (the kernel narrows it further)
  int fmt;           // split-operand kernels: k32 format code 1016 / 1032 / 1064 / 1128 / 2064, or column tile 64 / 128
  int pack;          // ssg_conv2d_split_bn: the split pack w_split must hold (fmt, with 2064 reading the pack of 1064), or 0
  int th, tw;        // pixel tile of the statistics epilogue (a bnpart row per tile), th = 0: none
  int ksplit;        // split-K slabs of the launch (1 = none): needs a workspace of ws_bytes
  int64_t ws_bytes;  // ssg_conv2d_workspace_bytes
  bool in_affine, bwd_stats;
  int id;            // ssg_conv2d_kernel_id
};

// One decision per descriptor: which kernel ssg_conv2d_f32 launches (mfma_only: ssg_conv2d_igemm_f32, no thin kernels), and
// everything the queries report about that launch.  Whether a family is eligible is decided in the family's file.
ConvPlan plan_conv(const ssg_conv_desc* d, bool mfma_only = false) {
  ConvPlan p{};
  p.rc = validate(d);
  if (p.rc != SSG_OK) return p;
  p.ksplit = 1;
  if (!mfma_only) {
    if ((p.variant = ssg_thin4_conv_kind(d))) { p.kind = KIND_THIN4; p.id = ssg_thin4_conv_id(d, p.variant); return p; }
    if ((p.variant = ssg_thin_conv_kind(d))) { p.kind = KIND_THIN; p.id = 9 + p.variant; return p; }
  }
  const ConvArgs& a = p.a = ssg_conv_to_args(d);
  const int v = p.variant = pick_variant(d);
  const bool dma = uses_dma(d), halo = uses_halo(a);
  // small grids split K over the idle CUs (fp32 halo tile, 16-byte output quads); never with bnpart (ssg_conv_halo_ksplit)
  const int ksplit = dma && halo && d->ldo % 4 == 0 && !((uintptr_t)d->out & 15) ? ssg_conv_halo_ksplit(a, v) : 1;
  if (d->Cout <= 32) p.fmt = halo ? ssg_conv_halo_k32_fmt(a) : 0;            // narrow k32 tiles (1016 / 1032), or nothing
  else if (!dma) p.fmt = 0;
  else if (d->parity_merge) p.fmt = ssg_conv_halo_x3_parity_ok(a) ? 64 : 0;
  else if (!halo) p.fmt = ssg_conv_dma_x3_bn(a);                               // 1x1, stride 2, parity classes: LDS-DMA pipeline
  else if (!ssg_conv_halo_x3_ok(a, v)) p.fmt = 0;
  else if ((p.fmt = ssg_conv_halo_k32_fmt(a))) {}                              // 32-channel chunks (grids that fill the chip, or forced)
  else p.fmt = ksplit > 1 ? 0 : ssg_conv_halo_x3_bn(a, v);                     // small grids keep split-K on the fp32 kernel
  p.pack = p.fmt == 2064 ? 1064 : p.fmt;
  if (d->w_split && p.fmt) p.kind = d->parity_merge ? KIND_PARITY : p.fmt >= 1000 ? KIND_K32 : halo ? KIND_HALO_X3 : KIND_DMA_X3;
  else p.kind = !dma ? KIND_REG : halo ? KIND_HALO : KIND_DMA;
  int hv, bn;
  switch (p.kind) {
    case KIND_K32:
      ssg_conv_halo_k32_tile(p.fmt, &p.th, &p.tw);
      p.id = p.fmt == 1128 ? 60 : p.fmt == 1064 ? 61 : p.fmt == 2064 ? 62 : p.fmt == 1016 ? 63 : 64;
      break;
    case KIND_PARITY:  p.th = 8; p.tw = 16; p.id = 42; break;
    case KIND_HALO_X3: p.th = 4; p.tw = 32; p.id = p.fmt == 128 ? 40 : 41; break;
    case KIND_DMA_X3:  p.th = 8; p.tw = 16; p.id = p.fmt == 128 ? 51 : 50; break;
    case KIND_HALO:
      hv = ssg_conv_halo_variant(a, v);
      p.id = 30 + hv;
      if (ksplit > 1) {
        p.ws_bytes = (int64_t)ksplit * d->N * d->GH * d->GW * ((d->Cout + 3) & ~3) * (int64_t)sizeof(float);
        if (d->ws && !d->bnpart && d->ws_bytes >= p.ws_bytes && !((uintptr_t)d->ws & 15)) p.ksplit = ksplit;
      } else {
        ssg_conv_halo_tile(hv, &p.th, &p.tw, &bn);
      }
      break;
    case KIND_DMA:     p.th = ssg_conv_dma_variant(a, v) == 1 ? 16 : 8; p.tw = 16; p.id = 20 + ssg_conv_dma_variant(a, v); break;
    default:           p.id = v; break;
  }
  p.in_affine = p.kind == KIND_K32 && ssg_conv_halo_k32_in_affine_ok(a, p.fmt);
  p.bwd_stats = p.kind == KIND_K32 && !d->res && !d->bias && d->act == SSG_ACT_NONE && !d->in_scale && ssg_conv_halo_k32_bwd_stats_ok(a, p.fmt);
  if (!mfma_only && ssg_conv1x1_k64_ok(d)) {     // the streaming kernel takes no bnpart: th / tw stay those of the kernel bnpart selects
    p.kind = KIND_1X1; p.id = 16; p.pack = 0;
  }
  return p;
}

int launch_plan(const ssg_conv_desc* d, const ConvPlan& p, void* stream) {
  if (p.rc != SSG_OK) return p.rc;
  SSG_REQUIRE(!d->in_scale || (d->in_shift && p.in_affine), SSG_EINVAL,
              "conv: in_scale on a descriptor whose kernel has no fused input transform (ssg_conv2d_in_affine_ok == 0)");
  SSG_REQUIRE(!d->bwd_x || (d->bnpart && d->bwd_scale && d->bwd_shift && d->bwd_mean && p.bwd_stats), SSG_EINVAL,
              "conv: bwd_x on a descriptor whose kernel has no backward-statistics epilogue (ssg_conv2d_bwd_stats_ok == 0), or without bnpart");
  SSG_REQUIRE(!d->bnpart || p.th, SSG_EINVAL, "conv: bnpart given but this shape has no statistics epilogue (ssg_conv2d_bnpart_rows == 0)");
  SSG_REQUIRE(!d->parity_merge || p.kind == KIND_PARITY, SSG_EINVAL,
              "conv: parity_merge needs a descriptor for which ssg_conv2d_split_bn reports 64 and its w_split pack");
  hipStream_t st = (hipStream_t)stream;
  ConvArgs a = p.a;
  switch (p.kind) {
    case KIND_THIN4: return ssg_thin4_conv_launch(d, p.variant, st);
    case KIND_THIN:  return ssg_thin_conv_launch(d, p.variant, st);
    case KIND_1X1:   return ssg_conv1x1_k64_launch(d, st);
    case KIND_HALO:
      if (p.ksplit > 1) { a.ws = d->ws; a.ksplit = p.ksplit; }
      return ssg_conv_igemm_halo_launch(a, p.variant, st);
    case KIND_DMA:   return ssg_conv_igemm_dma_launch(a, p.variant, st);
    case KIND_REG:
      if (p.variant == 0) return launch<128, 128, 2, 2>(a, st);
      if (p.variant == 1) return launch<256, 64, 4, 1>(a, st);
      return launch<256, 32, 4, 1>(a, st);
    default: break;
  }
  SSG_REQUIRE(ssg_aligned16(d->w_split), SSG_EALIGN, "conv: w_split alignment");
  a.w = (const float*)d->w_split;                        // operands split into bf16 terms on the bf16 matrix pipe
  switch (p.kind) {
    case KIND_K32:     return ssg_conv_igemm_halo_k32_launch(a, p.fmt, st);
    case KIND_PARITY:  return ssg_conv_igemm_halo_x3_parity_launch(a, st);
    case KIND_HALO_X3: return ssg_conv_igemm_halo_x3_launch(a, p.variant, st);
    default:           return ssg_conv_igemm_dma_x3_launch(a, st);
  }
}

}  // namespace

// The queries below read the plan of the descriptor as given (include/ssunet_hip.h).
extern "C" int ssg_conv2d_split_bn(const ssg_conv_desc* d) { const ConvPlan p = plan_conv(d); return p.rc == SSG_OK ? p.pack : 0; }
extern "C" int ssg_conv2d_in_affine_ok(const ssg_conv_desc* d) { const ConvPlan p = plan_conv(d); return p.rc == SSG_OK && p.in_affine; }
extern "C" int ssg_conv2d_bwd_stats_ok(const ssg_conv_desc* d) { const ConvPlan p = plan_conv(d); return p.rc == SSG_OK && p.bwd_stats; }
extern "C" int64_t ssg_conv2d_workspace_bytes(const ssg_conv_desc* d) { const ConvPlan p = plan_conv(d); return p.rc == SSG_OK ? p.ws_bytes : 0; }
extern "C" int ssg_conv2d_kernel_id(const ssg_conv_desc* d) { const ConvPlan p = plan_conv(d); return p.rc == SSG_OK ? p.id : p.rc; }

// SPADE backward (include/ssunet_hip.h): the launch ssg_conv2d_f32(d) makes for a descriptor without residual, with the product
// dout * (1 + gamma) added in its epilogue.  Only the thin-Cin kernels of conv_thin4.hip have that epilogue.
extern "C" int ssg_spade_dgrad_modulate_ok(const ssg_conv_desc* d) {
  if (!d || d->res || d->bias || d->act != SSG_ACT_NONE || d->in_scale || d->bwd_x || d->parity_merge) return 0;
  const ConvPlan p = plan_conv(d);
  return p.rc == SSG_OK && p.kind == KIND_THIN4 && ssg_thin4_conv_mod_ok(d, p.variant);
}

extern "C" int ssg_spade_dgrad_modulate_f32(const ssg_conv_desc* d, const float* dout, int lddout, const float* gamma, int ldg, void* stream) {
  SSG_REQUIRE(ssg_spade_dgrad_modulate_ok(d), SSG_EINVAL,
              "spade_dgrad_modulate: the launch of this descriptor has no modulated-residual epilogue (ssg_spade_dgrad_modulate_ok == 0)");
  const ConvPlan p = plan_conv(d);
  return ssg_thin4_conv_launch_mod(d, p.variant, dout, lddout, gamma, ldg, (hipStream_t)stream);
}

// rows of the batch-norm partial buffer the launch for `d` writes (one per pixel tile), or 0 when the kernel has no statistics
// epilogue (thin / register-staged kernels, split-K launches): the caller then runs ssg_bn_stats_f32 instead
extern "C" int ssg_conv2d_bnpart_rows(const ssg_conv_desc* d) {
  const ConvPlan p = plan_conv(d);
  if (p.rc != SSG_OK || !p.th) return 0;
  return ((d->GW + p.tw - 1) / p.tw) * ((d->GH + p.th - 1) / p.th) * d->N;
}

extern "C" int ssg_conv2d_igemm_f32(const ssg_conv_desc* d, void* stream) { return launch_plan(d, plan_conv(d, true), stream); }

extern "C" int ssg_conv2d_f32(const ssg_conv_desc* d, void* stream) {
  const ConvPlan p = plan_conv(d);
  SSG_REQUIRE(p.rc != SSG_OK || !d->parity_merge || p.pack == 64, SSG_EINVAL,
              "conv: parity_merge on a descriptor that has no merged-parity kernel (ssg_conv2d_split_bn != 64)");
  return launch_plan(d, p, stream);
}
