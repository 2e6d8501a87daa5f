// THE KEEP MASK of include/vsd.h in executable form: the integer weight of a mask byte, the blend of one byte, how a frame's pixels are
// divided among workgroups and walked (scalar head | 16-pixel vectors | scalar tail), where the 8 x 8 block of a latent pixel lies, and
// the host loops behind vsd_mask_blend_host / vsd_mask_latent_host.  Plain C++ that also compiles as HIP device code: the kernels of
// csrc/keep_mask.hip call the SAME mask_span / mask_walk / mask_block_at, and scripts/keep_mask_model.cpp runs them on the CPU under the
// sanitizers -- a wrong span or a vector access outside a frame is found there, not on the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MASK_HD __host__ __device__ __forceinline__
#else
#define MASK_HD inline
#endif

constexpr int MASK_MAX_SIDE = 16384;    // (= VSD_RESAMPLE_MAX_SIDE) N = h*w <= 2^28: 3*N fits an int
constexpr int MASK_MAX_FRAMES = 1024;   // (= VSD_MASK_MAX_FRAMES; blockIdx.y)
constexpr int MASK_WG_PIXELS = 4096, MASK_MAX_WGS = 64;  // a workgroup's span: at least this many pixels, until there are MASK_MAX_WGS of them
constexpr int MASK_VEC = 16;            // pixels of one vector step: 16 mask bytes, 48 bytes of either frame
constexpr int MASK_BLOCK = 8;           // a latent pixel covers MASK_BLOCK x MASK_BLOCK frame pixels
constexpr int MASK_FULL = MASK_BLOCK * MASK_BLOCK * 256;  // S of a fully restyled block = 16384

inline bool mask_args_ok(int frames, int h, int w) {
  return frames >= 1 && frames <= MASK_MAX_FRAMES && h >= 1 && w >= 1 && h <= MASK_MAX_SIDE && w <= MASK_MAX_SIDE;
}
inline bool mask_latent_args_ok(int frames, int h, int w) { return mask_args_ok(frames, h, w) && h % MASK_BLOCK == 0 && w % MASK_BLOCK == 0; }

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
MASK_HD int mask_weight(int m) { return m + (m >> 7); }  // 0..256, 256 exactly at m = 255
MASK_HD unsigned char mask_blend_byte(int in, int out, int a) { return (unsigned char)((in * (256 - a) + out * a + 128) >> 8); }  // (<= 255 * 256 + 128)
MASK_HD float mask_latent_weight(int S) { return (float)S / 16384.0f; }  // S <= 2^14: exact, and so is 1 - wl

// ---- how the n pixels of a frame are divided and walked ---------------------------------------------------------------------------------
MASK_HD int mask_wgs(int n) {
  const int g = (n + MASK_WG_PIXELS - 1) / MASK_WG_PIXELS;
  return g < 1 ? 1 : (g > MASK_MAX_WGS ? MASK_MAX_WGS : g);
}

// workgroup g of nwg: pixels [start, start + len) of the frame.  The spans are disjoint and cover it; a late workgroup's may be empty.
MASK_HD void mask_span(int n, int nwg, int g, int& start, int& len) {
  const int span = (n + nwg - 1) / nwg;
  start = g * span;
  len = start >= n ? 0 : (n - start < span ? n - start : span);
  if (len == 0) start = 0;
}

// `len` pixels whose mask bytes start at `maddr` and whose frame bytes start at `saddr` / `daddr` (3 bytes a pixel): pixels [0, head)
// one by one, then nvec steps of MASK_VEC pixels, the rest one by one.  A vector step reads 16 mask bytes and 48 bytes of either frame
// as 16-byte words, so it is taken only where the head that aligns the mask aligns both frames too; elsewhere nvec = 0 and every pixel is
// walked alone.
MASK_HD void mask_walk(uintptr_t maddr, uintptr_t saddr, uintptr_t daddr, int len, int& head, int& nvec) {
  head = (int)((16 - (maddr & 15)) & 15);
  if (head > len) head = len;
  const bool ok = (((saddr + 3 * (uintptr_t)head) | (daddr + 3 * (uintptr_t)head)) & 15) == 0;
  nvec = ok ? (len - head) / MASK_VEC : 0;
}

MASK_HD void mask_blend_pixel(const unsigned char* s, unsigned char* d, int m) {
  const int a = mask_weight(m);
  for (int c = 0; c < 3; ++c) d[c] = mask_blend_byte(s[c], d[c], a);
}

// byte offset, inside a [h][w] mask, of row r (0..7) of the block of latent pixel (y, x)
MASK_HD size_t mask_block_at(int w, int y, int x, int r) { return (size_t)(MASK_BLOCK * y + r) * w + (size_t)MASK_BLOCK * x; }

// ---- the contract as plain host loops ---------------------------------------------------------------------------------------------------
inline bool mask_blend_host(const unsigned char* src, unsigned char* dst, const unsigned char* mask, int frames, int h, int w) {
  if (!src || !dst || !mask || !mask_args_ok(frames, h, w)) return false;
  const size_t n = (size_t)frames * h * w;
  for (size_t p = 0; p < n; ++p) mask_blend_pixel(src + 3 * p, dst + 3 * p, mask[p]);
  return true;
}

inline bool mask_latent_host(const unsigned char* mask, int frames, int h, int w, float* weights) {
  if (!mask || !weights || !mask_latent_args_ok(frames, h, w)) return false;
  const int lh = h / MASK_BLOCK, lw = w / MASK_BLOCK;
  for (int f = 0; f < frames; ++f)
    for (int y = 0; y < lh; ++y)
      for (int x = 0; x < lw; ++x) {
        int S = 0;
        for (int r = 0; r < MASK_BLOCK; ++r) {
          const unsigned char* row = mask + (size_t)f * h * w + mask_block_at(w, y, x, r);
          for (int k = 0; k < MASK_BLOCK; ++k) S += mask_weight(row[k]);
        }
        weights[((size_t)f * lh + y) * lw + x] = mask_latent_weight(S);
      }
  return true;
}
