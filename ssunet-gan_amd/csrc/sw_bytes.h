// Byte access to the uint8 images of the sliding-window kernels (sliding_window.hip, sw_tta.hip) and the host check of a patch
// origin list.  Included inside each unit's anonymous namespace.
#pragma once

// Dword `idx` of the image as an aligned load; the last, partial dword of an image whose byte count is no multiple of 4 is put
// together from its bytes, and anything beyond reads as 0: no byte outside [0, total) is touched.
__device__ __forceinline__ uint32_t sw_ldw(const uint8_t* __restrict__ img, long long idx, long long total) {
  const long long b = idx * 4;
  if (b + 4 <= total) return *(const uint32_t*)(img + b);
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k)
    if (b + k < total) v |= (uint32_t)img[b + k] << (8 * k);
  return v;
}

// The NB (3 or 6) bytes at byte offset `b` (any alignment) as two dwords, from aligned loads.
template <int NB>
__device__ __forceinline__ void sw_bytes(const uint8_t* __restrict__ img, long long b, long long total, uint32_t& lo, uint32_t& hi) {
  const long long a = b >> 2;
  const int sh = 8 * (int)(b & 3);
  const uint32_t d0 = sw_ldw(img, a, total), d1 = sw_ldw(img, a + 1, total);
  lo = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
  hi = 0;
  if (NB > 4) {
    const uint32_t d2 = sw_ldw(img, a + 2, total);          // 3 + 6 bytes span at most three dwords
    hi = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
  }
}

// host copy of the origin list: every patch inside the image
static int sw_check_origins(const int32_t* org_host, int P, int p_size, int H, int W, const char* who) {
  for (int p = 0; p < P; ++p) {
    const int h1 = org_host[2 * p], w1 = org_host[2 * p + 1];
    SSG_REQUIRE(h1 >= 0 && w1 >= 0 && h1 <= H - p_size && w1 <= W - p_size, SSG_EINVAL,
                "%s: patch %d at (%d, %d), size %d, lies outside the %d x %d image", who, p, h1, w1, p_size, H, W);
  }
  return SSG_OK;
}
