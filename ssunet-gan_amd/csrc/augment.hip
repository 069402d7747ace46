// Training augmentation on the device, HBM-bound: uint8 source tiles + one parameter row and one 256-byte table
// per sample -> the network's input and target, NHWC fp32, in one launch per batch.  Rotate, Flip and Resize are one affine
// resampling (bilinear with 8-bit weights for the image, nearest for the masks), then the hue / saturation / value shift in
// integers, the brightness / contrast table, Normalize.  Everything up to the byte is integer arithmetic and the last two steps
// are one fp32 subtraction and one fp32 multiplication, so the result is tests/augment_ref.py bit for bit.
// ABI: include/ssunet_hip.h.
#include "common.h"

namespace {

constexpr int AUG_ROW = 16;            // int32 entries of a parameter row: m0 .. m5, flags, dh, ds, dv, 6 x 0
constexpr int AUG_FLAG_HSV = 1;

// (B, G, R) bytes -> H in 0 .. 179, S, V in 0 .. 255, every division rounded half up (augment_ref.hsv_from_bgr).
__device__ __forceinline__ void aug_hsv_from_bgr(int b, int g, int r, int& h, int& s, int& v) {
  v = max(max(b, g), r);
  const int mn = min(min(b, g), r);
  const int d = v - mn;
  const unsigned vs = (unsigned)max(v, 1);
  s = (int)((510u * (unsigned)d + vs) / (2u * vs));
  int num, off;
  if (v == r) { num = g - b; off = 0; }
  else if (v == g) { num = b - r; off = 60; }
  else { num = r - g; off = 120; }
  const unsigned dd = (unsigned)max(d, 1);
  // floor((60 num + d) / (2 d)) with num >= -d: 30 is added inside the division to keep the numerator positive
  h = (int)((unsigned)(60 * num + 61 * (int)dd) / (2u * dd)) - 30 + off;
  if (h < 0) h += 180;
  if (d == 0) h = 0;
}

// the inverse (augment_ref.bgr_from_hsv)
__device__ __forceinline__ void aug_bgr_from_hsv(int h, int s, int v, int& b, int& g, int& r) {
  const unsigned sec = (unsigned)h / 30u;
  const unsigned f = (unsigned)h - 30u * sec;
  const unsigned uv = (unsigned)v, us = (unsigned)s;
  const int p = (int)((2u * uv * (255u - us) + 255u) / 510u);
  const int q = (int)((2u * uv * (7650u - us * f) + 7650u) / 15300u);
  const int t = (int)((2u * uv * (7650u - us * (30u - f)) + 7650u) / 15300u);
  switch (sec) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// One thread per output pixel, lanes along the output row: the image pixel is one 16-byte store (1 KiB contiguous per wave),
// the target one or two.  The sample of a block, hence its parameter row, is uniform: the row arrives by scalar loads, the
// table is staged in LDS once per block.  Source bytes are read one by one (rows of 3 W bytes have no alignment) and only
// at addresses inside the source: a tap outside is the border constant.  Coordinates are int64 throughout.
__global__ __launch_bounds__(256) void augment_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, int H, int W, int C,
                                                      const int32_t* __restrict__ params, const uint8_t* __restrict__ lut, int out_h, int out_w,
                                                      int nb, int bd0, int bd1, int bd2, float mn0, float mn1, float mn2,
                                                      float rd0, float rd1, float rd2, float* __restrict__ out_img,
                                                      float* __restrict__ out_tgt, int ldt) {
  __shared__ uint8_t s_lut[256];
  const int n = (int)(blockIdx.x / (unsigned)nb);
  const int i = (int)(blockIdx.x % (unsigned)nb) * 256 + (int)threadIdx.x;
  s_lut[threadIdx.x] = lut[(size_t)n * 256 + threadIdx.x];
  __syncthreads();
  if (i >= out_h * out_w) return;
  const int32_t* row = params + (size_t)n * AUG_ROW;
  const int oy = i / out_w, ox = i - oy * out_w;
  const long long sx = (long long)row[0] * ox + (long long)row[1] * oy + row[2];
  const long long sy = (long long)row[3] * ox + (long long)row[4] * oy + row[5];
  const int flags = row[6];

  // image: four taps x three bytes
  const long long x0 = sx >> 16, y0 = sy >> 16;
  const int fx = (int)((sx >> 8) & 255), fy = (int)((sy >> 8) & 255);
  const int wgt[4] = {(256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy};
  const int bd[3] = {bd0, bd1, bd2};
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const long long x = x0 + (t & 1), y = y0 + (t >> 1);
    int px[3] = {bd[0], bd[1], bd[2]};
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const uint8_t* p = img + (((size_t)n * H + (size_t)y) * W + (size_t)x) * 3;
      px[0] = p[0];
      px[1] = p[1];
      px[2] = p[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += wgt[t] * px[c];
  }
  int v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = (acc[c] + (1 << 15)) >> 16;

  if (flags & AUG_FLAG_HSV) {                                  // uniform over the block
    int h, s, val;
    aug_hsv_from_bgr(v[0], v[1], v[2], h, s, val);
    h += row[7];
    h = h < 0 ? h + 180 : (h >= 180 ? h - 180 : h);
    s = min(max(s + row[8], 0), 255);
    val = min(max(val + row[9], 0), 255);
    aug_bgr_from_hsv(h, s, val, v[0], v[1], v[2]);
  }

  // table, then Normalize: (float(byte) - mean * 255) * (1 / (std * 255)), two fp32 roundings
  f32x4 o;
  o[0] = ((float)s_lut[v[0]] - mn0) * rd0;
  o[1] = ((float)s_lut[v[1]] - mn1) * rd1;
  o[2] = ((float)s_lut[v[2]] - mn2) * rd2;
  o[3] = 0.f;
  const size_t pix = (size_t)n * out_h * out_w + (size_t)i;
  *(f32x4*)(out_img + pix * 4) = o;

  // masks: nearest, border 0
  const long long nx = (sx + (1 << 15)) >> 16, ny = (sy + (1 << 15)) >> 16;
  const bool inside = nx >= 0 && nx < W && ny >= 0 && ny < H;
  const uint8_t* mp = mask + (((size_t)n * H + (size_t)(inside ? ny : 0)) * W + (size_t)(inside ? nx : 0)) * C;
  f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (inside && c < C) t0[c] = (float)mp[c];
  *(f32x4*)(out_tgt + pix * ldt) = t0;
  if (ldt == 8) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (inside && 4 + c < C) t1[c] = (float)mp[4 + c];
    *(f32x4*)(out_tgt + pix * ldt + 4) = t1;
  }
}

}  // namespace

extern "C" int ssg_augment_batch_u8_f32(const uint8_t* img, const uint8_t* mask, int N, int H, int W, int C, const int32_t* params,
                                        const int32_t* params_host, const uint8_t* lut, int out_h, int out_w,
                                        int border0, int border1, int border2, float mean0, float mean1, float mean2,
                                        float rdenom0, float rdenom1, float rdenom2, float* out_img, float* out_tgt, void* stream) {
  SSG_REQUIRE(img && mask && params && params_host && lut && out_img && out_tgt, SSG_EINVAL, "augment_batch: null pointer");
  SSG_REQUIRE(N > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0, SSG_EINVAL, "augment_batch: bad sizes (N %d, source %d x %d -> %d x %d)", N, H, W, out_h, out_w);
  SSG_REQUIRE(C >= 1 && C <= 8, SSG_EINVAL, "augment_batch: %d mask channels: 1 .. 8 are built", C);
  SSG_REQUIRE(border0 >= 0 && border0 <= 255 && border1 >= 0 && border1 <= 255 && border2 >= 0 && border2 <= 255, SSG_EINVAL,
              "augment_batch: border (%d, %d, %d) is no byte triple", border0, border1, border2);
  const long long nb = ssg_cdiv((long long)out_h * out_w, 256);
  SSG_REQUIRE((long long)out_h * out_w < (1ll << 31) && nb * N < (1ll << 31), SSG_EINVAL, "augment_batch: too large");
  for (int n = 0; n < N; ++n) {
    const int32_t* r = params_host + (size_t)n * AUG_ROW;
    SSG_REQUIRE((r[6] & ~AUG_FLAG_HSV) == 0, SSG_EINVAL, "augment_batch: sample %d: unknown flags 0x%x", n, (unsigned)r[6]);
    SSG_REQUIRE(r[7] >= -179 && r[7] <= 179 && r[8] >= -255 && r[8] <= 255 && r[9] >= -255 && r[9] <= 255, SSG_EINVAL,
                "augment_batch: sample %d: HSV shifts (%d, %d, %d) out of range", n, r[7], r[8], r[9]);
    for (int a = 0; a < 6; a += 3) {       // |m| <= 2^31 and extents < 2^31: each term < 2^62, summed in unsigned 64-bit
      const unsigned long long m0 = (unsigned long long)llabs((long long)r[a]), m1 = (unsigned long long)llabs((long long)r[a + 1]);
      const unsigned long long m2 = (unsigned long long)llabs((long long)r[a + 2]);
      const unsigned long long reach = m0 * (unsigned long long)(out_w - 1) + m1 * (unsigned long long)(out_h - 1) + m2 + (1ull << 15);
      SSG_REQUIRE(reach < (1ull << 62), SSG_EINVAL, "augment_batch: sample %d: the map overflows int64", n);
    }
  }
  SSG_REQUIRE(ssg_aligned16(out_img) && ssg_aligned16(out_tgt) && (((uintptr_t)params) & 3) == 0, SSG_EALIGN,
              "augment_batch: outputs 16-byte, parameter table 4-byte aligned");
  const int ldt = (C + 3) / 4 * 4;
  hipLaunchKernelGGL(augment_kernel, dim3((unsigned)(nb * N)), dim3(256), 0, (hipStream_t)stream, img, mask, H, W, C, params, lut, out_h, out_w,
                     (int)nb, border0, border1, border2, mean0, mean1, mean2, rdenom0, rdenom1, rdenom2, out_img, out_tgt, ldt);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}
