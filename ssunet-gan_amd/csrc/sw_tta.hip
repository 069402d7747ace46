// Flip / rotation test-time augmentation around the sliding-window forward, HBM-bound:
//   sw_gather_d4_kernel: sw_gather_kernel of sliding_window.hip with one of the 8 square symmetries folded into its index map;
//   sw_tta_reduce_kernel: K views' probabilities -> each mapped back, summed as a balanced tree in list order, times 1 / K.
// A view is a D4 code k in 0 .. 7, f = k >> 2, r = k & 3: T_k(a) = rot90(fliplr(a) if f else a, r), rot90 counter-clockwise
// (rot90(a)[i, j] = a[j, S - 1 - i]); T_k^-1(y) = fliplr(u) if f else u, u = rot90(y, 4 - r).  Both are "read pixel (sy, sx) for
// pixel (i, j)" with (sy, sx) = (rev_y(p), rev_x(q)), (p, q) = (j, i) if swap else (i, j), rev(t) = S - 1 - t or t: three bits per
// code and direction (sw_d4_map).  No atomics, one writer per output element.  ABI: include/ssunet_hip.h.
#include "common.h"

namespace {

#include "sw_bytes.h"

enum { SW_SWAP = 1, SW_REVY = 2, SW_REVX = 4 };

// The index map of T_k (inverse = 0: pixel (i, j) of T_k(a) is a[sy][sx]) or of T_k^-1 (inverse = 1) as SW_* bits.
//   T_k:    r = 0: a[i][f ? S-1-j : j]    r = 1: a[j][f ? i : S-1-i]    r = 2: a[S-1-i][f ? j : S-1-j]    r = 3: a[S-1-j][f ? S-1-i : i]
//   T_k^-1: r = 0: y[i][f ? S-1-j : j]    r = 1: y[f ? j : S-1-j][i]    r = 2: y[S-1-i][f ? j : S-1-j]    r = 3: y[f ? S-1-j : j][S-1-i]
__host__ __device__ __forceinline__ int sw_d4_map(int code, int inverse) {
  const int f = code >> 2, r = code & 3;
  if (r == 0) return f ? SW_REVX : 0;
  if (r == 2) return SW_REVY | (f ? 0 : SW_REVX);
  if (!inverse) return SW_SWAP | (r == 3 ? SW_REVY : 0) | ((r == 1) != (f != 0) ? SW_REVX : 0);
  return SW_SWAP | ((r == 1) != (f != 0) ? SW_REVY : 0) | (r == 3 ? SW_REVX : 0);
}

__device__ __forceinline__ void sw_d4_apply(int map, int S, int i, int j, int& sy, int& sx) {
  const int p = (map & SW_SWAP) ? j : i, q = (map & SW_SWAP) ? i : j;
  sy = (map & SW_REVY) ? S - 1 - p : p;
  sx = (map & SW_REVX) ? S - 1 - q : q;
}

// sw_gather_kernel with the unoriented patch read at map(oy, ox): one thread per output pixel, lanes along the OUTPUT row, every
// store one 16-byte pixel and 1 KiB contiguous per wave; the byte reads fall where the map puts them (down a column of the
// image under SW_SWAP).  The 2x2 box sum is symmetric in its four bytes and the normalisation is per pixel, so this is the
// oriented copy of what sw_gather_kernel writes, bit for bit.
template <int F>
__global__ __launch_bounds__(256) void sw_gather_d4_kernel(const uint8_t* __restrict__ img, int H, int W, const int32_t* __restrict__ org,
                                                           int out_size, int nb, int map, float m0, float m1, float m2, float r0, float r1,
                                                           float r2, float* __restrict__ out) {
  const int p = (int)(blockIdx.x / (unsigned)nb);
  const int i = (int)(blockIdx.x % (unsigned)nb) * 256 + (int)threadIdx.x;
  if (i >= out_size * out_size) return;
  const int h1 = org[2 * p], w1 = org[2 * p + 1];
  if (h1 < 0 || w1 < 0 || h1 > H - out_size * F || w1 > W - out_size * F) return;   // the entry point checked its host copy; never read outside
  const int oy = i / out_size, ox = i - oy * out_size;
  int sy, sx;
  sw_d4_apply(map, out_size, oy, ox, sy, sx);
  const long long total = (long long)H * W * 3;
  uint32_t v[3];
  if (F == 1) {
    uint32_t lo, hi;
    sw_bytes<3>(img, ((long long)(h1 + sy) * W + (w1 + sx)) * 3, total, lo, hi);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (lo >> (8 * c)) & 255u;
  } else {
    uint32_t lo0, hi0, lo1, hi1;
    const long long b = ((long long)(h1 + 2 * sy) * W + (w1 + 2 * sx)) * 3;
    sw_bytes<6>(img, b, total, lo0, hi0);
    sw_bytes<6>(img, b + (long long)W * 3, total, lo1, hi1);
    const uint64_t t = ((uint64_t)hi0 << 32) | lo0, u = ((uint64_t)hi1 << 32) | lo1;
#pragma unroll
    for (int c = 0; c < 3; ++c)                              // resize_u8 at 1/2: (a + b + c + d + 2) >> 2
      v[c] = ((uint32_t)((t >> (8 * c)) & 255u) + (uint32_t)((t >> (8 * c + 24)) & 255u) +
              (uint32_t)((u >> (8 * c)) & 255u) + (uint32_t)((u >> (8 * c + 24)) & 255u) + 2u) >> 2;
  }
  // normalize_imagenet then / 255: subtract, multiply, divide -- three correctly rounded fp32 operations, none fusable
  f32x4 o;
  o[0] = (((float)v[0] - m0) * r0) / 255.0f;
  o[1] = (((float)v[1] - m1) * r1) / 255.0f;
  o[2] = (((float)v[2] - m2) * r2) / 255.0f;
  o[3] = 0.f;
  *(f32x4*)(out + ((size_t)p * out_size * out_size + i) * 4) = o;
}

// One block per 32 x 32 output pixels of one sample and channel quad; thread (ty, tx) = (tid / 32, tid % 32) owns the pixels
// (i, j) = (oy0 + ty + 8 m, ox0 + tx), m = 0 .. 3: lanes along the output row, 16 B each.  A view without SW_SWAP is read where
// its map points: along a source row, forwards or backwards, 512 contiguous bytes per half wave.  A view with SW_SWAP (r odd)
// would be read down a source column; instead the thread loads the pixel of the TRANSPOSED position of the tile -- source-local
// (row ty + 8 m, column tx), again along a source row -- and the four pixels change hands through LDS: written at
// [ty + 8 m][tx], read at [tx][ty + 8 m], rows of 33 pixels.  Banks (16-B slots, 16 per 256-B bank row for ds_read_b128, 8 per
// 128 B for ds_write_b128): a write's 8-lane group holds 8 consecutive slots; a read's lane tx sits on slot (33 tx + i) % 16 =
// (tx + i) % 16, and each of the instruction's 16-lane groups holds 16 distinct tx % 16 -- no conflict by the bank rule.
// All K * 4 global loads are issued before the first LDS round trip.  The sum is the balanced tree in list order: a binary
// counter over partial sums, level l holding 2^l views.  `maps`: 3 bits per view, view k at bit 3 k.
constexpr int SW_TT = 32, SW_TP = 33;

template <int K>
__global__ __launch_bounds__(256) void sw_tta_reduce_kernel(const float* __restrict__ src, long long slab, int ld, unsigned maps, int C, int S,
                                                            int ntx, float* __restrict__ out, int ldo) {
  __shared__ f32x4 tile[SW_TT * SW_TP];
  const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;
  const int oy0 = (int)(blockIdx.x / (unsigned)ntx) * SW_TT, ox0 = (int)(blockIdx.x % (unsigned)ntx) * SW_TT;
  const int b = (int)blockIdx.y, c0 = 4 * (int)blockIdx.z;
  const int j = ox0 + tx;
  float* po = out + (size_t)b * S * S * ldo + c0;
  if (c0 >= C) {                                             // a quad of pad lanes only: +0.0, nothing read
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int i = oy0 + ty + 8 * m;
      if (i < S && j < S) *(f32x4*)(po + ((size_t)i * S + j) * ldo) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  const float* ps = src + (size_t)b * S * S * ld + c0;
  f32x4 raw[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int map = (int)(maps >> (3 * k)) & 7;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      // without SW_SWAP the thread's own pixel; with it the pixel whose source-local position is (ty + 8 m, tx)
      const int oi = (map & SW_SWAP) ? oy0 + tx : oy0 + ty + 8 * m, oj = (map & SW_SWAP) ? ox0 + ty + 8 * m : j;
      raw[k][m] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (oi < S && oj < S) {
        int sy, sx;
        sw_d4_apply(map, S, oi, oj, sy, sx);
        raw[k][m] = *(const f32x4*)(ps + (size_t)k * slab + ((size_t)sy * S + sx) * ld);
      }
    }
  }
  f32x4 part[4][4];                                          // [level][m]
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int map = (int)(maps >> (3 * k)) & 7;
    f32x4 cur[4];
    if (map & SW_SWAP) {                                     // block-uniform
      __syncthreads();                                       // the previous view's reads are done
#pragma unroll
      for (int m = 0; m < 4; ++m) tile[(ty + 8 * m) * SW_TP + tx] = raw[k][m];
      __syncthreads();
#pragma unroll
      for (int m = 0; m < 4; ++m) cur[m] = tile[tx * SW_TP + ty + 8 * m];
    } else {
#pragma unroll
      for (int m = 0; m < 4; ++m) cur[m] = raw[k][m];
    }
    int lvl = 0;
#pragma unroll
    for (int kk = k; kk & 1; kk >>= 1, ++lvl) {
#pragma unroll
      for (int m = 0; m < 4; ++m) cur[m] = part[lvl][m] + cur[m];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) part[lvl][m] = cur[m];
  }
  constexpr int TOP = K == 8 ? 3 : K == 4 ? 2 : K == 2 ? 1 : 0;
  constexpr float RK = 1.0f / (float)K;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int i = oy0 + ty + 8 * m;
    if (i >= S || j >= S) continue;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = K == 1 ? part[TOP][m][e] : part[TOP][m][e] * RK;
      o[e] = c0 + e < C ? v : 0.f;                           // a pad lane of src never reaches out
    }
    *(f32x4*)(po + ((size_t)i * S + j) * ldo) = o;
  }
}

}  // namespace

extern "C" int ssg_sw_gather_patches_d4_u8_f32(const uint8_t* img, int H, int W, const int32_t* org, const int32_t* org_host, int P,
                                               int p_size, int out_size, int orient, float mean0, float mean1, float mean2,
                                               float rdenom0, float rdenom1, float rdenom2, float* out, void* stream) {
  SSG_REQUIRE(img && org && org_host && out, SSG_EINVAL, "sw_gather_d4: null pointer");
  SSG_REQUIRE(orient >= 0 && orient <= 7, SSG_EINVAL, "sw_gather_d4: orient %d is no D4 code (0 .. 7)", orient);
  SSG_REQUIRE(P > 0 && H > 0 && W > 0 && p_size > 0 && out_size > 0, SSG_EINVAL, "sw_gather_d4: bad sizes (P %d, image %d x %d, patch %d -> %d)", P, H, W, p_size, out_size);
  SSG_REQUIRE(p_size == out_size || p_size == 2 * out_size, SSG_EINVAL, "sw_gather_d4: patch %d -> %d: only the factors 1 and 2 are built", p_size, out_size);
  if (int rc = sw_check_origins(org_host, P, p_size, H, W, "sw_gather_d4")) return rc;
  SSG_REQUIRE((((uintptr_t)img) & 3) == 0 && ssg_aligned16(out) && (((uintptr_t)org) & 3) == 0, SSG_EALIGN, "sw_gather_d4: image 4-byte, output 16-byte aligned");
  const long long nb = ssg_cdiv((long long)out_size * out_size, 256);
  SSG_REQUIRE((long long)out_size * out_size < (1ll << 31) && nb * P < (1ll << 31), SSG_EINVAL, "sw_gather_d4: too large");
  const dim3 grid((unsigned)(nb * P));
  const int map = sw_d4_map(orient, 0);
  if (p_size == out_size)
    hipLaunchKernelGGL(sw_gather_d4_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, img, H, W, org, out_size, (int)nb, map, mean0, mean1, mean2, rdenom0, rdenom1, rdenom2, out);
  else
    hipLaunchKernelGGL(sw_gather_d4_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, img, H, W, org, out_size, (int)nb, map, mean0, mean1, mean2, rdenom0, rdenom1, rdenom2, out);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

extern "C" int ssg_sw_tta_reduce_f32(const float* src, int64_t slab, int ld, int K, const int32_t* codes, int B, int C, int S,
                                     float* out, int ldo, void* stream) {
  SSG_REQUIRE(src && codes && out, SSG_EINVAL, "sw_tta_reduce: null pointer");
  SSG_REQUIRE(K == 1 || K == 2 || K == 4 || K == 8, SSG_EINVAL, "sw_tta_reduce: %d views: 1, 2, 4 or 8 are built", K);
  unsigned maps = 0, seen = 0;
  for (int k = 0; k < K; ++k) {
    SSG_REQUIRE(codes[k] >= 0 && codes[k] <= 7, SSG_EINVAL, "sw_tta_reduce: view %d has code %d, no D4 code (0 .. 7)", k, codes[k]);
    SSG_REQUIRE(!(seen >> codes[k] & 1u), SSG_EINVAL, "sw_tta_reduce: code %d is repeated", codes[k]);
    seen |= 1u << codes[k];
    maps |= (unsigned)sw_d4_map(codes[k], 1) << (3 * k);
  }
  SSG_REQUIRE(B > 0 && C > 0 && S > 0, SSG_EINVAL, "sw_tta_reduce: bad sizes (B %d, C %d, S %d)", B, C, S);
  SSG_REQUIRE(C <= ld && C <= ldo, SSG_EINVAL, "sw_tta_reduce: %d channels in pixels of %d (src) and %d (out) floats", C, ld, ldo);
  SSG_REQUIRE(ld % 4 == 0 && ldo % 4 == 0 && slab % 4 == 0 && ssg_aligned16(src) && ssg_aligned16(out), SSG_EALIGN,
              "sw_tta_reduce: ld %d, ldo %d, view stride %lld: multiples of 4, tensors 16-byte aligned", ld, ldo, (long long)slab);
  SSG_REQUIRE(slab >= (int64_t)B * S * S * ld || K == 1, SSG_EINVAL, "sw_tta_reduce: view stride %lld is less than one view (%d x %d x %d x %d)",
              (long long)slab, B, S, S, ld);
  const long long nt = ssg_cdiv(S, SW_TT);
  SSG_REQUIRE(nt * nt < (1ll << 31) && B <= 65535 && ldo / 4 <= 65535, SSG_EINVAL, "sw_tta_reduce: too large");
  const dim3 grid((unsigned)(nt * nt), (unsigned)B, (unsigned)(ldo / 4));
#define SW_TTA_LAUNCH(KK) \
  hipLaunchKernelGGL(sw_tta_reduce_kernel<KK>, grid, dim3(256), 0, (hipStream_t)stream, src, (long long)slab, ld, maps, C, S, (int)nt, out, ldo)
  if (K == 1) SW_TTA_LAUNCH(1);
  else if (K == 2) SW_TTA_LAUNCH(2);
  else if (K == 4) SW_TTA_LAUNCH(4);
  else SW_TTA_LAUNCH(8);
#undef SW_TTA_LAUNCH
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}
