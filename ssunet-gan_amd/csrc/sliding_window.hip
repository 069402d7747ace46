// Sliding-window inference around the generator forward (aerial_image_segmentation_api.py, BASELINE config 5), HBM-bound:
//   sw_gather_kernel: uint8 BGR image + patch origins -> network input (crop, 2x2 box resize, double normalisation), NHWC ld 4;
//   sw_merge_kernel:  per-patch probabilities -> {0, 255} class masks at image resolution (uint8 round trip, 2x bilinear,
//                     threshold, overlap vote, threshold);
//   sw_gather_labels_kernel: uint8 BGR label image + patch origins -> per-class {0, 1} patches (mask_convert), NHWC ld 4,
//                     merged by sw_merge_kernel like probabilities: the ground-truth branch;
//   sw_mask_counts_kernel: two uint8 mask sets -> per-class pixel counts (both, prediction, ground truth), added to a buffer.
// All restate integer / single-rounding arithmetic of the host functions get_patched_input, patch_merge and mask_convert and
// are meant to match them bit for bit.  ABI: include/ssunet_hip.h.
#include "common.h"

namespace {

#include "sw_bytes.h"

// One thread per output pixel, lanes along the patch row: every store is one 16-byte pixel, 1 KiB contiguous per wave.
// F = p_size / out_size.  The origin of the block's patch is wave-uniform (scalar loads, once per thread).
template <int F>
__global__ __launch_bounds__(256) void sw_gather_kernel(const uint8_t* __restrict__ img, int H, int W, const int32_t* __restrict__ org,
                                                        int out_size, int nb, float m0, float m1, float m2, float r0, float r1, float r2,
                                                        float* __restrict__ out) {
  const int p = (int)(blockIdx.x / (unsigned)nb);
  const int i = (int)(blockIdx.x % (unsigned)nb) * 256 + (int)threadIdx.x;
  if (i >= out_size * out_size) return;
  const int h1 = org[2 * p], w1 = org[2 * p + 1];
  if (h1 < 0 || w1 < 0 || h1 > H - out_size * F || w1 > W - out_size * F) return;   // the entry point checked its host copy; never read outside
  const int oy = i / out_size, ox = i - oy * out_size;
  const long long total = (long long)H * W * 3;
  uint32_t v[3];
  if (F == 1) {
    uint32_t lo, hi;
    sw_bytes<3>(img, ((long long)(h1 + oy) * W + (w1 + ox)) * 3, total, lo, hi);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (lo >> (8 * c)) & 255u;
  } else {
    uint32_t lo0, hi0, lo1, hi1;
    const long long b = ((long long)(h1 + 2 * oy) * W + (w1 + 2 * ox)) * 3;
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

// (uint8)(p * 255) of patch_merge for p in [0, 1]
__device__ __forceinline__ int sw_u8(float p) { return (int)(p * 255.0f) & 255; }

// One thread per image pixel, one block per 256-pixel piece of an image row; for each class quad a thread walks the patches and
// counts, with the patch's weight, those whose resized uint8 map exceeds 127 at its pixel.  Gather form: no atomics, every output
// byte has one writer.  The origin / weight lists are read 64 entries at a time, one entry per lane, and handed round the wave
// with v_readlane: the patch loop itself reads no list from memory, and a patch that misses the block's row is skipped by a
// scalar branch.  F = p_size / S; at F = 2 the four taps of resize_u8's 2x bilinear carry weights (9, 3, 3, 1) / 16, so
// floor(v + 0.5) > 127  <=>  9a + 3b + 3c + d >= 2040 in integers.
template <int F>
__global__ __launch_bounds__(256) void sw_merge_kernel(const float* __restrict__ probs, int ld, int P, int C, int S,
                                                       const int32_t* __restrict__ org, const int32_t* __restrict__ wt, int H, int W, int nbx,
                                                       uint8_t* __restrict__ out) {
  const int y = (int)(blockIdx.x / (unsigned)nbx);
  const int x = (int)(blockIdx.x % (unsigned)nbx) * 256 + (int)threadIdx.x;
  const int lane = (int)threadIdx.x & 63;
  const int p_size = S * F;
  for (int c0 = 0; c0 < C; c0 += 4) {
    int k[4] = {0, 0, 0, 0}, n = 0;
    for (int base = 0; base < P; base += 64) {
      int vh = 0, vw = 0, vm = 0;
      if (base + lane < P) {
        vh = org[2 * (base + lane)];
        vw = org[2 * (base + lane) + 1];
        vm = wt[base + lane];
      }
      const int cnt = P - base < 64 ? P - base : 64;
      for (int j = 0; j < cnt; ++j) {
        const int h1 = __builtin_amdgcn_readlane(vh, j), w1 = __builtin_amdgcn_readlane(vw, j), m = __builtin_amdgcn_readlane(vm, j);
        const int ly = y - h1;
        if (ly < 0 || ly >= p_size || m == 0) continue;                   // wave-uniform
        const int lx = x - w1;
        if (x >= W || lx < 0 || lx >= p_size) continue;
        const float* pp = probs + (size_t)(base + j) * S * S * ld + c0;
        int hit[4];
        if (F == 1) {
          const f32x4 a = *(const f32x4*)(pp + ((size_t)ly * S + lx) * ld);
#pragma unroll
          for (int e = 0; e < 4; ++e) hit[e] = sw_u8(a[e]) > 127;
        } else {
          // resize_u8 at 2: output 2i blends (i - 1, i), output 2i + 1 blends (i, i + 1), 0.25 / 0.75, clamped at the edges
          const int iy = ly >> 1, ix = lx >> 1;
          const int jy = (ly & 1) ? (iy + 1 < S ? iy + 1 : S - 1) : (iy > 0 ? iy - 1 : 0);
          const int jx = (lx & 1) ? (ix + 1 < S ? ix + 1 : S - 1) : (ix > 0 ? ix - 1 : 0);
          const f32x4 a = *(const f32x4*)(pp + ((size_t)iy * S + ix) * ld), b = *(const f32x4*)(pp + ((size_t)iy * S + jx) * ld);
          const f32x4 c = *(const f32x4*)(pp + ((size_t)jy * S + ix) * ld), d = *(const f32x4*)(pp + ((size_t)jy * S + jx) * ld);
#pragma unroll
          for (int e = 0; e < 4; ++e) hit[e] = 9 * sw_u8(a[e]) + 3 * sw_u8(b[e]) + 3 * sw_u8(c[e]) + sw_u8(d[e]) >= 2040;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] += hit[e] ? m : 0;
        n += m;
      }
    }
    if (x < W) {
      const double dn = (double)(n == 0 ? 1 : n);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < C)                                                   // patch_merge's own fp64 operations: (merged / div * 255) -> uint8 -> > 127
          out[((size_t)(c0 + e) * H + y) * W + x] = (int)((double)k[e] / dn * 255.0) > 127 ? 255 : 0;
    }
  }
}

// The class a label pixel selects, as a bit set: its three bytes in memory order as one 24-bit value against the palette of
// mask_convert -- class 0 (255, 255, 255), class 1 (255, 0, 0), class 2 (0, 0, 255).
__device__ __forceinline__ void sw_label_hits(uint32_t px, int (&k)[3]) {
  px &= 0xffffffu;
  k[0] += px == 0xffffffu;
  k[1] += px == 0x0000ffu;
  k[2] += px == 0xff0000u;
}

// sw_gather_kernel's shape on a label image: one thread per output pixel, one 16-byte store each.  k = selected pixels of the
// F x F source box; F = 1 stores k, F = 2 stores k >= 2: resize_u8 at 1/2 of a {0, 255} mask is (255 k + 2) >> 2 in
// {0, 64, 128, 191, 255}, of which post_process_resized_mask keeps 128 and above.  Lanes C .. 3 are +0.0.
template <int F>
__global__ __launch_bounds__(256) void sw_gather_labels_kernel(const uint8_t* __restrict__ img, int H, int W, const int32_t* __restrict__ org,
                                                               int out_size, int nb, int C, float* __restrict__ out) {
  const int p = (int)(blockIdx.x / (unsigned)nb);
  const int i = (int)(blockIdx.x % (unsigned)nb) * 256 + (int)threadIdx.x;
  if (i >= out_size * out_size) return;
  const int h1 = org[2 * p], w1 = org[2 * p + 1];
  if (h1 < 0 || w1 < 0 || h1 > H - out_size * F || w1 > W - out_size * F) return;   // the entry point checked its host copy; never read outside
  const int oy = i / out_size, ox = i - oy * out_size;
  const long long total = (long long)H * W * 3;
  int k[3] = {0, 0, 0};
  if (F == 1) {
    uint32_t lo, hi;
    sw_bytes<3>(img, ((long long)(h1 + oy) * W + (w1 + ox)) * 3, total, lo, hi);
    sw_label_hits(lo, k);
  } else {
    uint32_t lo0, hi0, lo1, hi1;
    const long long b = ((long long)(h1 + 2 * oy) * W + (w1 + 2 * ox)) * 3;
    sw_bytes<6>(img, b, total, lo0, hi0);
    sw_bytes<6>(img, b + (long long)W * 3, total, lo1, hi1);
    const uint64_t t = ((uint64_t)hi0 << 32) | lo0, u = ((uint64_t)hi1 << 32) | lo1;
    sw_label_hits((uint32_t)t, k);
    sw_label_hits((uint32_t)(t >> 24), k);
    sw_label_hits((uint32_t)u, k);
    sw_label_hits((uint32_t)(u >> 24), k);
  }
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (c < C) o[c] = (F == 1 ? k[c] : (k[c] >= 2)) ? 1.f : 0.f;
  *(f32x4*)(out + ((size_t)p * out_size * out_size + i) * 4) = o;
}

typedef uint32_t sw_u32x4 __attribute__((ext_vector_type(4)));

// Per class (blockIdx.y) the pixels with pred > 127 and gt > 127, with pred > 127, with gt > 127 -- bit 7 of each byte, three
// popcounts per 8 bytes -- added into counts[class][3].  A plane starts at any byte: the bytes before the prediction plane's
// first 16-byte boundary and behind the last whole 16 are taken one by one, the rest 16 per thread and set; where the two
// planes sit differently inside their 16-byte lines the whole plane goes byte by byte.  Blocks own contiguous chunks; sums are
// reduced over the wave, then over the block's four waves in LDS, and three 64-bit integer atomics per block reach memory.
__global__ __launch_bounds__(256) void sw_mask_counts_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, long long HW,
                                                             unsigned long long* __restrict__ counts) {
  const int c = (int)blockIdx.y;
  const uint8_t* p = pred + (size_t)c * HW;
  const uint8_t* g = gt + (size_t)c * HW;
  long long head = (long long)((16 - ((uintptr_t)p & 15)) & 15);
  if (head > HW) head = HW;
  const bool vec = (((uintptr_t)(g + head)) & 15) == 0;
  const long long nv = vec ? (HW - head) / 16 : 0;           // 16-byte pieces, both planes aligned
  const long long nbyte = HW - 16 * nv;                      // head and tail bytes (everything when not vec)
  unsigned long long s[3] = {0, 0, 0};
  SSG_CHUNK_LOOP(q, nv) {
    const sw_u32x4 a = *(const sw_u32x4*)(p + head + 16 * q), b = *(const sw_u32x4*)(g + head + 16 * q);
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const uint64_t x = ((((uint64_t)a[e + 1] << 32) | a[e]) & 0x8080808080808080ull);
      const uint64_t y = ((((uint64_t)b[e + 1] << 32) | b[e]) & 0x8080808080808080ull);
      s[0] += (unsigned)__popcll(x & y);
      s[1] += (unsigned)__popcll(x);
      s[2] += (unsigned)__popcll(y);
    }
  }
  SSG_CHUNK_LOOP(j, nbyte) {
    const long long i = j < head ? j : j + 16 * nv;
    const unsigned x = p[i] >> 7, y = g[i] >> 7;
    s[0] += x & y;
    s[1] += x;
    s[2] += y;
  }
  __shared__ unsigned long long part[4][3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s[e] += __shfl_xor(s[e], m, 64);
  }
  if ((threadIdx.x & 63) == 0)
    for (int e = 0; e < 3; ++e) part[threadIdx.x >> 6][e] = s[e];
  __syncthreads();
  if (threadIdx.x < 3) {
    const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (v) atomicAdd(counts + 3 * c + threadIdx.x, v);
  }
}

}  // namespace

extern "C" int ssg_sw_gather_patches_u8_f32(const uint8_t* img, int H, int W, const int32_t* org, const int32_t* org_host, int P,
                                            int p_size, int out_size, float mean0, float mean1, float mean2,
                                            float rdenom0, float rdenom1, float rdenom2, float* out, void* stream) {
  SSG_REQUIRE(img && org && org_host && out, SSG_EINVAL, "sw_gather: null pointer");
  SSG_REQUIRE(P > 0 && H > 0 && W > 0 && p_size > 0 && out_size > 0, SSG_EINVAL, "sw_gather: bad sizes (P %d, image %d x %d, patch %d -> %d)", P, H, W, p_size, out_size);
  SSG_REQUIRE(p_size == out_size || p_size == 2 * out_size, SSG_EINVAL, "sw_gather: patch %d -> %d: only the factors 1 and 2 are built", p_size, out_size);
  if (int rc = sw_check_origins(org_host, P, p_size, H, W, "sw_gather")) return rc;
  SSG_REQUIRE((((uintptr_t)img) & 3) == 0 && ssg_aligned16(out) && (((uintptr_t)org) & 3) == 0, SSG_EALIGN, "sw_gather: image 4-byte, output 16-byte aligned");
  const long long nb = ssg_cdiv((long long)out_size * out_size, 256);
  SSG_REQUIRE((long long)out_size * out_size < (1ll << 31) && nb * P < (1ll << 31), SSG_EINVAL, "sw_gather: too large");
  const dim3 grid((unsigned)(nb * P));
  if (p_size == out_size)
    hipLaunchKernelGGL(sw_gather_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, img, H, W, org, out_size, (int)nb, mean0, mean1, mean2, rdenom0, rdenom1, rdenom2, out);
  else
    hipLaunchKernelGGL(sw_gather_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, img, H, W, org, out_size, (int)nb, mean0, mean1, mean2, rdenom0, rdenom1, rdenom2, out);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

extern "C" int ssg_sw_merge_masks_f32_u8(const float* probs, int ld, int P, int C, int S, const int32_t* org, const int32_t* org_host,
                                         const int32_t* weight, int p_size, int H, int W, uint8_t* out, void* stream) {
  SSG_REQUIRE(probs && org && org_host && weight && out, SSG_EINVAL, "sw_merge: null pointer");
  SSG_REQUIRE(P > 0 && C > 0 && S > 0 && H > 0 && W > 0 && p_size > 0, SSG_EINVAL, "sw_merge: bad sizes (P %d, C %d, S %d, image %d x %d, patch %d)", P, C, S, H, W, p_size);
  SSG_REQUIRE(p_size == S || p_size == 2 * S, SSG_EINVAL, "sw_merge: %d -> patch %d: only the factors 1 and 2 are built", S, p_size);
  SSG_REQUIRE(ld % 4 == 0 && ld >= C, SSG_EALIGN, "sw_merge: ld %d for %d classes", ld, C);
  if (int rc = sw_check_origins(org_host, P, p_size, H, W, "sw_merge")) return rc;
  SSG_REQUIRE(ssg_aligned16(probs) && (((uintptr_t)org) & 3) == 0 && (((uintptr_t)weight) & 3) == 0, SSG_EALIGN, "sw_merge: probabilities 16-byte aligned");
  const long long nbx = ssg_cdiv(W, 256);
  SSG_REQUIRE(nbx * H < (1ll << 31), SSG_EINVAL, "sw_merge: too large");
  const dim3 grid((unsigned)(nbx * H));
  if (p_size == S)
    hipLaunchKernelGGL(sw_merge_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, probs, ld, P, C, S, org, weight, H, W, (int)nbx, out);
  else
    hipLaunchKernelGGL(sw_merge_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, probs, ld, P, C, S, org, weight, H, W, (int)nbx, out);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

// mask_convert over every patch of a label image (aerial_image_segmentation_api.py:220-236,394-406)
extern "C" int ssg_sw_gather_labels_u8_f32(const uint8_t* label, int H, int W, const int32_t* org, const int32_t* org_host, int P,
                                           int p_size, int out_size, int C, float* out, void* stream) {
  SSG_REQUIRE(label && org && org_host && out, SSG_EINVAL, "sw_gather_labels: null pointer");
  SSG_REQUIRE(P > 0 && H > 0 && W > 0 && p_size > 0 && out_size > 0, SSG_EINVAL, "sw_gather_labels: bad sizes (P %d, image %d x %d, patch %d -> %d)", P, H, W, p_size, out_size);
  SSG_REQUIRE(p_size == out_size || p_size == 2 * out_size, SSG_EINVAL, "sw_gather_labels: patch %d -> %d: only the factors 1 and 2 are built", p_size, out_size);
  SSG_REQUIRE(C >= 1 && C <= 3, SSG_EINVAL, "sw_gather_labels: %d classes: the label palette has 3 colours", C);
  if (int rc = sw_check_origins(org_host, P, p_size, H, W, "sw_gather_labels")) return rc;
  SSG_REQUIRE((((uintptr_t)label) & 3) == 0 && ssg_aligned16(out) && (((uintptr_t)org) & 3) == 0, SSG_EALIGN, "sw_gather_labels: image 4-byte, output 16-byte aligned");
  const long long nb = ssg_cdiv((long long)out_size * out_size, 256);
  SSG_REQUIRE((long long)out_size * out_size < (1ll << 31) && nb * P < (1ll << 31), SSG_EINVAL, "sw_gather_labels: too large");
  const dim3 grid((unsigned)(nb * P));
  if (p_size == out_size)
    hipLaunchKernelGGL(sw_gather_labels_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, label, H, W, org, out_size, (int)nb, C, out);
  else
    hipLaunchKernelGGL(sw_gather_labels_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, label, H, W, org, out_size, (int)nb, C, out);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

// intersection / prediction / ground-truth pixel counts of the two mask sets (aerial_image_segmentation_api.py:220-236,394-406)
extern "C" int ssg_sw_mask_counts_u8(const uint8_t* pred, const uint8_t* gt, int C, int64_t HW, uint64_t* counts, void* stream) {
  SSG_REQUIRE(pred && gt && counts, SSG_EINVAL, "sw_mask_counts: null pointer");
  SSG_REQUIRE(C >= 1 && C <= 65535 && HW > 0, SSG_EINVAL, "sw_mask_counts: bad sizes (%d classes of %lld pixels)", C, (long long)HW);
  SSG_REQUIRE((((uintptr_t)counts) & 7) == 0, SSG_EALIGN, "sw_mask_counts: counts 8-byte aligned");
  // 64 KiB of each set per block, at most 1024 blocks per class: the three atomics that end a block land on nine adjacent words,
  // and at 2048^2 they, not the loads, were the time above the launch floor (768 blocks: +5.5 us, 192 blocks: +2.4 us)
  long long gx = ssg_cdiv(HW, 65536);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(sw_mask_counts_kernel, dim3((unsigned)gx, (unsigned)C), dim3(256), 0, (hipStream_t)stream, pred, gt, (long long)HW,
                     (unsigned long long*)counts);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}
