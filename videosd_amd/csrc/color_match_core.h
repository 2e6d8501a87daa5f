// THE COLOUR CONTRACT of include/vsd.h in executable form: how a frame is divided among workgroups and walked, the arithmetic of one
// LUT entry, and the host loops behind vsd_color_match_host.  Plain C++ that also compiles as HIP device code: the kernels of
// csrc/color_match.hip call the SAME color_span / color_walk / color_lut_entry, and scripts/color_match_model.cpp runs them on the CPU
// under the sanitizers -- a wrong span or a vector access outside a frame is found there, not on the device.
//
// The device form in three launches (no global atomics, no memset, no host sync):
//   1. histograms: workgroup g of color_wgs(N) counts bytes [start, start + len) of one frame (color_span) of src and of dst into
//                  LDS and stores partial[frame][g][6][256] (0..2: src by channel, 3..5: dst).
//   2. LUT:        one workgroup per frame sums the partials, forms prefix sums / moments, and thread v writes lut[frame][c][v].
//   3. apply:      the same spans as launch 1; dst[i] = lut[i % 3][dst[i]].
// The channel of a byte is its offset in the frame mod 3.  A span is walked as scalar head | 16-byte vectors | scalar tail (color_walk),
// because a frame starts at any byte offset.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define COLOR_HD __host__ __device__ __forceinline__
#else
#define COLOR_HD inline
#endif

// Every fp64 operation of the contract is rounded on its own.  __dmul_rn / __dadd_rn are plain `*` / `+` in the HIP headers, which the
// compiler may still contract into an fma: so contraction is switched off inside the functions below (and color_match.hip is built
// with -ffp-contract=off, as is every host program that includes this header: see build.py and scripts/color_match_model.cpp).
#if defined(__clang__)
#define COLOR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define COLOR_NO_CONTRACT
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define COLOR_DMUL(A_, B_) __dmul_rn((A_), (B_))
#define COLOR_DADD(A_, B_) __dadd_rn((A_), (B_))
#define COLOR_DDIV(A_, B_) __ddiv_rn((A_), (B_))
#define COLOR_DSQRT(A_) __dsqrt_rn((A_))
#else
#define COLOR_DMUL(A_, B_) ((A_) * (B_))
#define COLOR_DADD(A_, B_) ((A_) + (B_))
#define COLOR_DDIV(A_, B_) ((A_) / (B_))
#define COLOR_DSQRT(A_) sqrt((A_))
#endif

constexpr int COLOR_HIST = 0, COLOR_MEANSTD = 1;  // (= VSD_COLOR_HIST, VSD_COLOR_MEANSTD)
constexpr int COLOR_MAX_SIDE = 16384;             // (= VSD_RESAMPLE_MAX_SIDE)
constexpr int COLOR_MAX_PIXELS = 1 << 23;         // (= VSD_COLOR_MAX_PIXELS) N^2 * 255^2 < 2^62; 3 * N < 2^25: byte offsets of a frame fit an int
constexpr int COLOR_MAX_FRAMES = 1024;            // (= VSD_COLOR_MAX_FRAMES; blockIdx.y)
constexpr int COLOR_MAX_AMOUNT = 256;
constexpr int COLOR_WG_BYTES = 16384, COLOR_MAX_WGS = 64;  // a workgroup's span: at least this many bytes, until there are COLOR_MAX_WGS of them
constexpr int COLOR_PARTIAL = 6 * 256;                     // u32 words of one workgroup's partial histograms

inline bool color_args_ok(int h, int w, int mode) {
  return h >= 1 && w >= 1 && h <= COLOR_MAX_SIDE && w <= COLOR_MAX_SIDE && (int64_t)h * w <= COLOR_MAX_PIXELS && (mode == COLOR_HIST || mode == COLOR_MEANSTD);
}

// ---- how a frame of `nbytes` = 3 * N bytes is divided and walked ---------------------------------------------------------------------
COLOR_HD int color_wgs(int nbytes) {
  const int g = (nbytes + COLOR_WG_BYTES - 1) / COLOR_WG_BYTES;
  return g < 1 ? 1 : (g > COLOR_MAX_WGS ? COLOR_MAX_WGS : g);
}

// workgroup g of nwg: bytes [start, start + len) of the frame.  The spans are disjoint and cover it; a late workgroup's may be empty.
// (nwg * span <= nbytes + nwg * nwg: no overflow)
COLOR_HD void color_span(int nbytes, int nwg, int g, int& start, int& len) {
  const int span = (nbytes + nwg - 1) / nwg;
  start = g * span;
  len = start >= nbytes ? 0 : (nbytes - start < span ? nbytes - start : span);
  if (len == 0) start = 0;
}

// `len` bytes from address `addr`: bytes [0, head) one by one, nvec 16-byte vectors from head (an aligned address), the rest one by one
COLOR_HD void color_walk(uintptr_t addr, int len, int& head, int& nvec) {
  head = (int)((16 - (addr & 15)) & 15);
  if (head > len) head = len;
  nvec = (len - head) >> 4;
}

inline int64_t color_workspace_bytes(int frames, int h, int w) {
  if (frames < 1 || frames > COLOR_MAX_FRAMES || !color_args_ok(h, w, COLOR_HIST)) return 0;
  const int64_t one = (int64_t)color_wgs(h * w * 3) * COLOR_PARTIAL * 4 + 768;  // partial u32 [nwg][6][256], then (after ALL partials) lut u8 [3][256]
  return (frames * one + 255) / 256 * 256;
}

// ---- one LUT entry -------------------------------------------------------------------------------------------------------------------
// HIST: the smallest u with 2 * Cs[u] >= 2 * cd - hd, where cd = Cd[v], hd = Hd[v] (hd <= cd, so the right side is >= 0).  Cs is
// non-decreasing with Cs[255] = N >= cd: the answer exists, and eight halvings of [0, 255] find it.
COLOR_HD int color_match_hist(const uint32_t* Cs, uint32_t cd, uint32_t hd) {
  const uint32_t need = 2u * cd - hd;
  int lo = 0, hi = 255;
  for (int trip = 0; trip < 8; ++trip) {
    const int mid = (lo + hi) >> 1;
    if (2u * Cs[mid] >= need)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// MEANSTD: the gain from the moments (n = N; ss, qs, sd, qd = S and Q of src and dst)
COLOR_HD double color_gain(int64_t n, int64_t ss, int64_t qs, int64_t sd, int64_t qd) {
  COLOR_NO_CONTRACT
  const int64_t vs = n * qs - ss * ss, vd = n * qd - sd * sd;
  if (vd == 0) return 0.0;
  const double r = COLOR_DSQRT(COLOR_DDIV((double)vs, (double)vd));
  return r < 4.0 ? r : 4.0;
}

COLOR_HD int color_match_meanstd(int64_t n, int64_t ss, int64_t sd, double g, int v) {
  COLOR_NO_CONTRACT
  const double t = COLOR_DADD(COLOR_DDIV(COLOR_DADD((double)ss, COLOR_DMUL(g, (double)(n * v - sd))), (double)n), 0.5);
  const double f = floor(t);  // |t| < 2^35: the comparisons and the conversion below are exact
  return f < 0.0 ? 0 : (f > 255.0 ? 255 : (int)f);
}

COLOR_HD int color_clamp_amount(int a) { return a < 0 ? 0 : (a > COLOR_MAX_AMOUNT ? COLOR_MAX_AMOUNT : a); }

COLOR_HD unsigned char color_blend(int v, int m, int a) { return (unsigned char)((v * (256 - a) + m * a + 128) >> 8); }  // (<= 255 * 256 + 128)

// ---- the contract as plain host loops -------------------------------------------------------------------------------------------------
// H: counts [6][256] (0..2 src by channel, 3..5 dst) of a frame of n pixels -> lut [3][256]
inline void color_build_lut(const uint32_t (*H)[256], int64_t n, int mode, int amount, unsigned char (*lut)[256]) {
  for (int c = 0; c < 3; ++c) {
    uint32_t Cs[256], Cd[256];
    int64_t ss = 0, qs = 0, sd = 0, qd = 0;
    uint32_t as = 0, ad = 0;
    for (int v = 0; v < 256; ++v) {
      Cs[v] = as += H[c][v];
      Cd[v] = ad += H[3 + c][v];
      ss += (int64_t)v * H[c][v];
      qs += (int64_t)v * v * H[c][v];
      sd += (int64_t)v * H[3 + c][v];
      qd += (int64_t)v * v * H[3 + c][v];
    }
    const double g = mode == COLOR_MEANSTD ? color_gain(n, ss, qs, sd, qd) : 0.0;
    for (int v = 0; v < 256; ++v) {
      const int m = mode == COLOR_MEANSTD ? color_match_meanstd(n, ss, sd, g, v) : color_match_hist(Cs, Cd[v], H[3 + c][v]);
      lut[c][v] = color_blend(v, m, amount);
    }
  }
}

inline bool color_match_host(const unsigned char* src, unsigned char* dst, int h, int w, int mode, int amount) {
  if (!src || !dst || !color_args_ok(h, w, mode) || amount < 0 || amount > COLOR_MAX_AMOUNT) return false;
  const int nbytes = h * w * 3;
  static_assert(sizeof(uint32_t[6][256]) == COLOR_PARTIAL * 4, "one partial");
  uint32_t H[6][256] = {};
  for (int i = 0; i < nbytes; ++i) {
    H[i % 3][src[i]] += 1;
    H[3 + i % 3][dst[i]] += 1;
  }
  unsigned char lut[3][256];
  color_build_lut(H, (int64_t)h * w, mode, amount, lut);
  for (int i = 0; i < nbytes; ++i) dst[i] = lut[i % 3][dst[i]];
  return true;
}
