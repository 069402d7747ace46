// Confidence maps of sliding-window inference, beside sliding_window.hip:
//   sw_merge_scores_kernel: per-patch probabilities -> per pixel and class the score S in 0 .. 255, the number of first-stage
//                     levels t in 0 .. 254 at which patch_merge, thresholding every patch at t instead of 127, turns the pixel
//                     on (S > 127 is sw_merge_kernel's mask); or, given one level per class, the masks S > level;
//   sw_score_hist_kernel: a score map and a ground-truth mask set -> per class and ground-truth bit the 256-bin histogram of S,
//                     from which every threshold's intersection / prediction / ground-truth counts follow by suffix sums.
// Integer arithmetic and patch_merge's own fp64 expression only: meant to match the host functions patch_merge_scores and
// score_hist bit for bit.  ABI: include/ssunet_hip.h.
#include "common.h"

namespace {

#include "sw_bytes.h"

__device__ __forceinline__ int sws_u8(float p) { return (int)(p * 255.0f) & 255; }   // (uint8)(p * 255) of patch_merge for p in [0, 1]

struct SwLevels { uint8_t v[64]; };                                                   // mask mode: the level of each class

// One walk over the patch list, sw_merge_kernel's: for every patch that covers pixel (y, x) with weight m > 0, visit(s, m) with
// s[e] the resized uint8 value of class c0 + e in the walk's own scale -- at F = 1 the byte r itself, at F = 2 the tap sum
// 9a + 3b + 3c + d of resize_u8's 2x bilinear (taps (9, 3, 3, 1) / 16, edge-clamped), of which r = floor(v + 0.5) = (s + 8) >> 4.
// The lists go round the wave 64 entries at a time by v_readlane (every lane of the wave must be here); a patch that misses
// the row is skipped by a scalar branch.
template <int F, class Visit>
__device__ __forceinline__ void sws_walk(const float* __restrict__ probs, int ld, int P, int S, const int32_t* __restrict__ org,
                                         const int32_t* __restrict__ wt, int y, int x, int W, int lane, int c0, Visit&& visit) {
  const int p_size = S * F;
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
      int s[4];
      if (F == 1) {
        const f32x4 a = *(const f32x4*)(pp + ((size_t)ly * S + lx) * ld);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = sws_u8(a[e]);
      } else {
        // resize_u8 at 2: output 2i blends (i - 1, i), output 2i + 1 blends (i, i + 1), 0.25 / 0.75, clamped at the edges
        const int iy = ly >> 1, ix = lx >> 1;
        const int jy = (ly & 1) ? (iy + 1 < S ? iy + 1 : S - 1) : (iy > 0 ? iy - 1 : 0);
        const int jx = (lx & 1) ? (ix + 1 < S ? ix + 1 : S - 1) : (ix > 0 ? ix - 1 : 0);
        const f32x4 a = *(const f32x4*)(pp + ((size_t)iy * S + ix) * ld), b = *(const f32x4*)(pp + ((size_t)iy * S + jx) * ld);
        const f32x4 c = *(const f32x4*)(pp + ((size_t)jy * S + ix) * ld), d = *(const f32x4*)(pp + ((size_t)jy * S + jx) * ld);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = 9 * sws_u8(a[e]) + 3 * sws_u8(b[e]) + 3 * sws_u8(c[e]) + sws_u8(d[e]);
      }
      visit(s, m);
    }
  }
}

// r >= level in the walk's scale: (s + 8) >> 4 >= L  <=>  s >= 16 L - 8
template <int F>
__device__ __forceinline__ int sws_scale(int level) { return F == 1 ? level : 16 * level - 8; }

// patch_merge's second stage in its own fp64 operations: (merged / div * 255) -> uint8 -> > 127
__device__ __forceinline__ bool sws_vote(int k, int n) { return (int)((double)k / (double)(n == 0 ? 1 : n) * 255.0) > 127; }

// The smallest k that passes the vote among n > 0: the vote is monotone in k (one rounded division, one rounded product) and
// true at k = n, so an estimate near 128 n / 255 is walked to the boundary with the vote itself -- two or three fp64 divisions
// per pixel instead of one per class and bisection step.  No k passes at n = 0.
__device__ __forceinline__ int sws_kmin(int n) {
  if (n <= 0) return 0x7fffffff;
  int k = (int)((double)n * (128.0 / 255.0));
  while (k > 0 && sws_vote(k - 1, n)) --k;
  while (!sws_vote(k, n)) ++k;
  return k;
}

constexpr int SWS_CACHE = 16;                                             // (r, m) pairs a thread keeps: 32 KiB of LDS per block

// sw_merge_kernel's geometry: one thread per image pixel, one block per 256-pixel piece of an image row, every output byte one
// writer, no atomics, integer accumulation.
// MASK: one walk counting the weight with r > level, the vote as {0, 255}: sw_merge_kernel with the level in a register.
// Score mode: the voters {r >= L} shrink as L grows, so the levels L in 1 .. 255 that pass the vote are a prefix and S is its end,
// the weighted upper quantile of the covering patches' r at weight kmin (sws_kmin).  ONE walk stores the thread's (r of the four
// classes, m) pairs in its own LDS column, up to SWS_CACHE of them -- 16 covers the shipped geometry without dedupe (36 patches, 16
// on an interior pixel), 4 with it -- and an 8-step bisection per class over (lo, hi) = (0, 256), "L = lo passes or lo = 0, L = hi
// does not", then reads the pairs back instead of the probabilities.  A wave in which some pixel has more pairs than that bisects
// over the patch list itself, one walk per step at the four classes' own midpoints: exact for any number of covering patches
// (overlap 0.75 without dedupe: 64), eight times the loads.  A thread reads only the LDS it wrote: no barrier.  DESIGN.md 3.27.
template <int F, bool MASK>
__global__ __launch_bounds__(256) void sw_merge_scores_kernel(const float* __restrict__ probs, int ld, int P, int C, int S,
                                                              const int32_t* __restrict__ org, const int32_t* __restrict__ wt, int H, int W,
                                                              int nbx, SwLevels thr, uint8_t* __restrict__ out) {
  const int y = (int)(blockIdx.x / (unsigned)nbx);
  const int x = (int)(blockIdx.x % (unsigned)nbx) * 256 + (int)threadIdx.x;
  const int lane = (int)threadIdx.x & 63;
  for (int c0 = 0; c0 < C; c0 += 4) {
    int res[4];
    if constexpr (MASK) {
      int lv[4], k[4] = {0, 0, 0, 0}, n = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) lv[e] = sws_scale<F>((int)thr.v[(c0 + e) & 63] + 1);
      sws_walk<F>(probs, ld, P, S, org, wt, y, x, W, lane, c0, [&](const int (&s)[4], int m) {
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] += s[e] >= lv[e] ? m : 0;
        n += m;
      });
#pragma unroll
      for (int e = 0; e < 4; ++e) res[e] = sws_vote(k[e], n) ? 255 : 0;
    } else {
      __shared__ uint2 cache[SWS_CACHE][256];
      int cnt = 0, n = 0;
      sws_walk<F>(probs, ld, P, S, org, wt, y, x, W, lane, c0, [&](const int (&s)[4], int m) {
        uint32_t r = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) r |= (uint32_t)(F == 1 ? s[e] : (s[e] + 8) >> 4) << (8 * e);
        if (cnt < SWS_CACHE) cache[cnt][threadIdx.x] = make_uint2(r, (uint32_t)m);
        ++cnt;
        n += m;
      });
      const int kmin = sws_kmin(n);
      int lo[4] = {0, 0, 0, 0}, hi[4] = {256, 256, 256, 256};
      if (!__any(cnt > SWS_CACHE)) {                                      // wave-uniform
#pragma unroll 1
        for (int step = 0; step < 8; ++step) {
          int mid[4], k[4] = {0, 0, 0, 0};
#pragma unroll
          for (int e = 0; e < 4; ++e) mid[e] = (lo[e] + hi[e]) >> 1;
          for (int j = 0; j < cnt; ++j) {
            const uint2 v = cache[j][threadIdx.x];
#pragma unroll
            for (int e = 0; e < 4; ++e) k[e] += (int)((v.x >> (8 * e)) & 255u) >= mid[e] ? (int)v.y : 0;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool on = k[e] >= kmin;
            lo[e] = on ? mid[e] : lo[e];
            hi[e] = on ? hi[e] : mid[e];
          }
        }
      } else {
#pragma unroll 1
        for (int step = 0; step < 8; ++step) {                            // uniform trip count: the walk needs the whole wave
          int mid[4], lv[4], k[4] = {0, 0, 0, 0};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            mid[e] = (lo[e] + hi[e]) >> 1;
            lv[e] = sws_scale<F>(mid[e]);
          }
          sws_walk<F>(probs, ld, P, S, org, wt, y, x, W, lane, c0, [&](const int (&s)[4], int m) {
#pragma unroll
            for (int e = 0; e < 4; ++e) k[e] += s[e] >= lv[e] ? m : 0;
          });
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool on = k[e] >= kmin;
            lo[e] = on ? mid[e] : lo[e];
            hi[e] = on ? hi[e] : mid[e];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) res[e] = lo[e];
    }
    if (x < W) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < C) out[((size_t)(c0 + e) * H + y) * W + x] = (uint8_t)res[e];
    }
  }
}

typedef uint32_t sws_u32x4 __attribute__((ext_vector_type(4)));

// One add per run of equal bins among a thread's consecutive bytes: flat regions of a score map (0 and 255 are the common
// values of a confident model) cost one LDS atomic per 16 bytes instead of 16 on one address.
struct SwRun {
  unsigned* h;
  unsigned bin, len;
  __device__ __forceinline__ void put(unsigned b) {
    if (b == bin) { ++len; return; }
    if (len) atomicAdd(h + bin, len);
    bin = b;
    len = 1;
  }
  __device__ __forceinline__ void flush() { if (len) atomicAdd(h + bin, len); len = 0; }
};

// Per class (blockIdx.y) and g = gt > 127 the histogram of the score bytes, added into hist[class][g][256] (64-bit).  Planes
// start at any byte and HW is any number, handled as in sw_mask_counts_kernel: a byte head up to the score plane's first 16-byte
// boundary, 16 bytes per thread where both planes are then aligned, a byte tail; byte by byte throughout where they sit
// differently inside their 16-byte lines.  Blocks own contiguous chunks of fewer than 2^32 bytes (the entry point sizes the
// grid), so a 32-bit bin cannot overflow.  Each wave has its own 2 x 256 bins in LDS (8 KiB per block: the four waves do not
// meet on an address); after the barrier thread t sums the four copies of bins t and 256 + t and adds what is non-zero to memory,
// a wave's 64 adds on 512 contiguous bytes.
__global__ __launch_bounds__(256) void sw_score_hist_kernel(const uint8_t* __restrict__ scores, const uint8_t* __restrict__ gt, long long HW,
                                                            unsigned long long* __restrict__ hist) {
  __shared__ unsigned bins[4][512];
  const int c = (int)blockIdx.y;
  for (int i = (int)threadIdx.x; i < 4 * 512; i += 256) (&bins[0][0])[i] = 0;
  __syncthreads();
  const uint8_t* p = scores + (size_t)c * HW;
  const uint8_t* g = gt + (size_t)c * HW;
  long long head = (long long)((16 - ((uintptr_t)p & 15)) & 15);
  if (head > HW) head = HW;
  const bool vec = (((uintptr_t)(g + head)) & 15) == 0;
  const long long nv = vec ? (HW - head) / 16 : 0;           // 16-byte pieces, both planes aligned
  const long long nbyte = HW - 16 * nv;                      // head and tail bytes (everything when not vec)
  SwRun run = {bins[threadIdx.x >> 6], 0u, 0u};
  SSG_CHUNK_LOOP(q, nv) {
    const sws_u32x4 a = *(const sws_u32x4*)(p + head + 16 * q), b = *(const sws_u32x4*)(g + head + 16 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int s = 0; s < 32; s += 8) run.put(((a[e] >> s) & 255u) | (((b[e] >> (s + 7)) & 1u) << 8));
    }
  }
  SSG_CHUNK_LOOP(j, nbyte) {
    const long long i = j < head ? j : j + 16 * nv;
    run.put((unsigned)p[i] | ((unsigned)(g[i] >> 7) << 8));
  }
  run.flush();
  __syncthreads();
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int b = half * 256 + (int)threadIdx.x;
    const unsigned long long v = (unsigned long long)bins[0][b] + bins[1][b] + bins[2][b] + bins[3][b];
    if (v) atomicAdd(hist + (size_t)c * 512 + b, v);
  }
}

}  // namespace

// the score map of patch_merge (thr_host == NULL) or its masks at one first-stage level per class
extern "C" int ssg_sw_merge_scores_f32_u8(const float* probs, int ld, int P, int C, int S, const int32_t* org, const int32_t* org_host,
                                          const int32_t* weight, int p_size, int H, int W, const int32_t* thr_host, uint8_t* out, void* stream) {
  SSG_REQUIRE(probs && org && org_host && weight && out, SSG_EINVAL, "sw_merge_scores: null pointer");
  SSG_REQUIRE(P > 0 && C > 0 && S > 0 && H > 0 && W > 0 && p_size > 0, SSG_EINVAL, "sw_merge_scores: bad sizes (P %d, C %d, S %d, image %d x %d, patch %d)", P, C, S, H, W, p_size);
  SSG_REQUIRE(p_size == S || p_size == 2 * S, SSG_EINVAL, "sw_merge_scores: %d -> patch %d: only the factors 1 and 2 are built", S, p_size);
  SSG_REQUIRE(ld % 4 == 0 && ld >= C, SSG_EALIGN, "sw_merge_scores: ld %d for %d classes", ld, C);
  if (int rc = sw_check_origins(org_host, P, p_size, H, W, "sw_merge_scores")) return rc;
  SwLevels thr = {};
  if (thr_host) {
    SSG_REQUIRE(C <= 64, SSG_EINVAL, "sw_merge_scores: levels for %d classes: at most 64 classes take levels", C);
    for (int c = 0; c < C; ++c) {
      SSG_REQUIRE(thr_host[c] >= 0 && thr_host[c] <= 254, SSG_EINVAL, "sw_merge_scores: level %d of class %d lies outside 0 .. 254", thr_host[c], c);
      thr.v[c] = (uint8_t)thr_host[c];
    }
  }
  SSG_REQUIRE(ssg_aligned16(probs) && (((uintptr_t)org) & 3) == 0 && (((uintptr_t)weight) & 3) == 0, SSG_EALIGN, "sw_merge_scores: probabilities 16-byte aligned");
  const long long nbx = ssg_cdiv(W, 256);
  SSG_REQUIRE(nbx * H < (1ll << 31), SSG_EINVAL, "sw_merge_scores: too large");
  const dim3 grid((unsigned)(nbx * H));
#define SWS_LAUNCH(F, MASK)                                                                                                        \
  hipLaunchKernelGGL((sw_merge_scores_kernel<F, MASK>), grid, dim3(256), 0, (hipStream_t)stream, probs, ld, P, C, S, org, weight, H, W, \
                     (int)nbx, thr, out)
  if (p_size == S) {
    if (thr_host) SWS_LAUNCH(1, true); else SWS_LAUNCH(1, false);
  } else {
    if (thr_host) SWS_LAUNCH(2, true); else SWS_LAUNCH(2, false);
  }
#undef SWS_LAUNCH
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}

// histogram of a score map per class and ground-truth bit
extern "C" int ssg_sw_score_hist_u8(const uint8_t* scores, const uint8_t* gt, int C, int64_t HW, int64_t* hist, void* stream) {
  SSG_REQUIRE(scores && gt && hist, SSG_EINVAL, "sw_score_hist: null pointer");
  SSG_REQUIRE(C >= 1 && C <= 65535 && HW > 0, SSG_EINVAL, "sw_score_hist: bad sizes (%d classes of %lld pixels)", C, (long long)HW);
  SSG_REQUIRE((((uintptr_t)hist) & 7) == 0, SSG_EALIGN, "sw_score_hist: histogram 8-byte aligned");
  // 64 KiB of each plane per block, at most 1024 blocks per class as in sw_mask_counts; more only where a block's chunk would
  // reach 2^31 bytes, so that a 32-bit LDS bin cannot overflow whatever the plane holds
  long long gx = ssg_cdiv(HW, 65536);
  if (gx > 1024) gx = 1024;
  if (ssg_cdiv(HW, gx) >= (1ll << 31)) gx = ssg_cdiv(HW, 1ll << 30);
  SSG_REQUIRE(gx < (1ll << 31), SSG_EINVAL, "sw_score_hist: too large");
  hipLaunchKernelGGL(sw_score_hist_kernel, dim3((unsigned)gx, (unsigned)C), dim3(256), 0, (hipStream_t)stream, scores, gt, (long long)HW,
                     (unsigned long long*)hist);
  SSG_LAUNCH_CHECK();
  return SSG_OK;
}
