// THE BLUR CONTRACT of include/vsd.h in executable form: the two rounding expressions, the clamp, the check of a tap table, which source
// rows and byte columns a workgroup's tile needs and how a row of it is walked (single bytes where a tap is clamped | groups of four
// bytes from aligned 4-byte words elsewhere), and the host loops behind vsd_gauss_blur_host.  Plain C++ that also compiles as HIP
// device code: the kernel of csrc/blur.hip calls the SAME blur_tile / blur_group_words / blur_h_byte / blur_h_group / blur_v_*, and
// scripts/blur_model.cpp runs them on the CPU under the sanitizers over buffers of exactly the needed size -- a tile one halo row short
// or a word read outside the operand is found there, not on the device.
//
// A row is C*w BYTES: byte b of a row is channel b % C of pixel b / C, and tap i of an unclamped byte is byte b + i*C, so C = 3 is the
// code of C = 1 with a tap stride of three bytes.  Accumulators are uint32_t: for a valid table every sum stays below 2^31 (vsd.h), and
// for a table the host check would refuse they wrap, which is defined -- unspecified bytes, never undefined behaviour.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BLUR_HD __host__ __device__ __forceinline__
#else
#define BLUR_HD inline
#endif

constexpr int BLUR_MAX_SIDE = 16384;   // (= VSD_RESAMPLE_MAX_SIDE) C*h*w <= 3 * 2^28: a frame's bytes fit an int
constexpr int BLUR_MAX_FRAMES = 1024;  // (blockIdx.z)
constexpr int BLUR_MAX_RADIUS = 32;    // (= VSD_BLUR_MAX_RADIUS)
constexpr int BLUR_ONE = 16384;        // (= VSD_BLUR_ONE) the taps' sum
constexpr int BLUR_TAPS = 34;          // {R, w_0 .. w_32}
// A workgroup's tile: BLUR_TILE_H rows of BLUR_TILE_W byte columns.  Its LDS image has room for the halo of R = 32 above and below:
// (64 + 64) * 32 u16 = 8 KB, far below the 64 KB at which two workgroups still fit a CU's 160 KB.  A design choice, not a measured
// optimum, with one measured point behind the width: every lane walks a chain of dependent loads, so the launch lives on waves in
// flight, and a narrow tile costs no load more (a group reads its own span whatever the tile) while five 512 x 512 frames become 1920
// workgroups, not 480 (profiles/blur_stage.txt has both).  A taller tile would redo fewer halo rows per output row (2 x at R = 32
// here, 1.16 x at R = 5).
constexpr int BLUR_TILE_W = 32, BLUR_TILE_H = 64;
constexpr int BLUR_LDS_ROWS = BLUR_TILE_H + 2 * BLUR_MAX_RADIUS;
constexpr int BLUR_GROUP = 4;  // bytes of one group: one 4-byte word of the destination, four u16 of the LDS image
constexpr int BLUR_MAX_TILES = 1 << 23;  // tiles of one call: 256 threads each, below 2^31 threads
static_assert(BLUR_LDS_ROWS * BLUR_TILE_W * 2 <= 64 * 1024 && BLUR_TILE_W % BLUR_GROUP == 0, "LDS image");

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
BLUR_HD uint32_t blur_round_h(uint32_t H) { return (H + 32u) >> 6; }          // H <= 255 * 16384: h16 = 0..65280, the value times 256
BLUR_HD uint32_t blur_round_v(uint32_t V) { return (V + (1u << 21)) >> 22; }  // V <= 65280 * 16384: V + 2^21 < 2^31; 0..255
// acc + wt * v.  A valid tap is at most 16384 and v at most 65280: both fit 24 bits, so the device takes its full-rate 24-bit multiply-add
// (a tap the host check would refuse may lose its upper bits there: unspecified bytes, as the contract says).
BLUR_HD uint32_t blur_mac(uint32_t acc, uint32_t wt, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(wt, v) + acc;
#else
  return acc + wt * v;
#endif
}
BLUR_HD int blur_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
BLUR_HD int blur_radius(int r) { return r < 1 ? 1 : (r > BLUR_MAX_RADIUS ? BLUR_MAX_RADIUS : r); }  // what the kernel does with ANY table

inline bool blur_taps_ok(const int32_t* t) {
  if (!t || t[0] < 1 || t[0] > BLUR_MAX_RADIUS) return false;
  int64_t sum = 0;
  for (int i = 0; i <= BLUR_MAX_RADIUS; ++i) {
    if (t[1 + i] < 0 || (i > t[0] && t[1 + i] != 0)) return false;
    sum += (i ? 2 : 1) * (int64_t)t[1 + i];
  }
  return sum == BLUR_ONE;
}

inline bool blur_args_ok(int frames, int h, int w, int channels) {
  return frames >= 1 && frames <= BLUR_MAX_FRAMES && h >= 1 && w >= 1 && h <= BLUR_MAX_SIDE && w <= BLUR_MAX_SIDE && (channels == 1 || channels == 3);
}

// ---- a workgroup's tile -----------------------------------------------------------------------------------------------------------------
BLUR_HD int blur_tiles_x(int w, int C) { return (C * w + BLUR_TILE_W - 1) / BLUR_TILE_W; }
BLUR_HD int blur_tiles_y(int h) { return (h + BLUR_TILE_H - 1) / BLUR_TILE_H; }

struct BlurTile {
  int c0, c1;        // byte columns [c0, c1) of a row
  int y0, y1;        // output rows [y0, y1)
  int rows;          // LDS rows: y1 - y0 + 2R; LDS row r holds source row blur_clamp(y0 - R + r, h)
  int body0, body1;  // byte columns [body0, body1) of the tile no tap of which is clamped (may be empty); the others are walked alone
};

BLUR_HD BlurTile blur_tile(int h, int w, int C, int R, int tx, int ty) {
  BlurTile t;
  const int rb = C * w;
  t.c0 = tx * BLUR_TILE_W;
  t.c1 = t.c0 + BLUR_TILE_W < rb ? t.c0 + BLUR_TILE_W : rb;
  t.y0 = ty * BLUR_TILE_H;
  t.y1 = t.y0 + BLUR_TILE_H < h ? t.y0 + BLUR_TILE_H : h;
  t.rows = t.y1 - t.y0 + 2 * R;
  const int lo = R * C, hi = (w - R) * C;  // bytes of pixels R .. w - 1 - R
  t.body0 = t.c0 > lo ? t.c0 : lo;
  t.body1 = t.c1 < hi ? t.c1 : hi;
  if (t.body1 < t.body0) t.body1 = t.body0;
  return t;
}
BLUR_HD int blur_lds_src_row(const BlurTile& t, int R, int r, int h) { return blur_clamp(t.y0 - R + r, h); }

// The group of bytes [b, b + 4) of the row at address `row` goes through words when none of its taps is clamped and every aligned word
// the walk below touches -- from the word of byte b - R*C to the word AFTER that of byte b + R*C -- lies inside the operand
// [lo, hi): a word never reaches outside `src`, whatever its alignment.  Elsewhere the group's bytes are walked alone.
BLUR_HD bool blur_group_words(const BlurTile& t, int b, uintptr_t row, uintptr_t lo, uintptr_t hi, int R, int C) {
  if (b < t.body0 || b + BLUR_GROUP > t.body1) return false;
  const uintptr_t first = (row + (uintptr_t)(b - R * C)) & ~(uintptr_t)3, last = (row + (uintptr_t)(b + R * C)) & ~(uintptr_t)3;
  return first >= lo && last + 8 <= hi;
}

// one byte alone: channel b % C of pixel b / C, every tap's pixel index clamped.  tap(k) = w_k.
template <class Tap>
BLUR_HD uint32_t blur_h_byte(const unsigned char* row, int b, int w, int C, int R, Tap tap) {
  const int x = b / C, c = b - x * C;
  uint32_t H = 0;
  for (int i = -R; i <= R; ++i) H = blur_mac(H, (uint32_t)tap(i < 0 ? -i : i), row[blur_clamp(x + i, w) * C + c]);
  return blur_round_h(H);
}

// four bytes at once (blur_group_words holds): out[k] = h16 of byte b + k.  The four source bytes of tap i start at byte b + i*C, at any
// alignment: they are cut from a window of two aligned words that slides on by C < 4 bytes per tap.  word(a) = the 4-byte word at the
// 4-byte-aligned address a.
template <class Tap, class Word>
BLUR_HD void blur_h_group(uintptr_t row, int b, int C, int R, Tap tap, Word word, uint32_t out[BLUR_GROUP]) {
  uintptr_t q = row + (uintptr_t)(b - R * C), a = q & ~(uintptr_t)3;
  uint32_t lo = word(a), hi = word(a + 4);
  uint32_t H[BLUR_GROUP] = {0, 0, 0, 0};
  for (int i = -R; i <= R; ++i) {
    const uint32_t four = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (unsigned)(q & 3)));
    const uint32_t wt = (uint32_t)tap(i < 0 ? -i : i);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < BLUR_GROUP; ++k) H[k] = blur_mac(H[k], wt, (four >> (8 * k)) & 255u);
    q += (uintptr_t)C;
    if (i < R && (q & ~(uintptr_t)3) != a) {  // (not behind the last tap: the word after the window's is never read for nothing)
      a += 4;
      lo = hi;
      hi = word(a + 4);
    }
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < BLUR_GROUP; ++k) out[k] = blur_round_h(H[k]);
}

// the vertical pass of one byte column: `col` points at LDS row (y - y0) of the column -- source row y - R --, rows `pitch` u16 apart
template <class Tap>
BLUR_HD unsigned char blur_v_byte(const uint16_t* col, int pitch, int R, Tap tap) {
  uint32_t V = 0;
  for (int j = -R; j <= R; ++j) V = blur_mac(V, (uint32_t)tap(j < 0 ? -j : j), col[(R + j) * pitch]);
  return (unsigned char)blur_round_v(V);
}

// ---- the contract as plain host loops ---------------------------------------------------------------------------------------------------
inline bool blur_host(const unsigned char* src, unsigned char* dst, int frames, int h, int w, int C, const int32_t* taps) {
  if (!src || !dst || !blur_args_ok(frames, h, w, C) || !blur_taps_ok(taps)) return false;
  const int R = taps[0], rb = C * w;
  auto tap = [taps](int k) { return taps[1 + k]; };
  std::vector<uint16_t> h16((size_t)h * rb);
  for (int f = 0; f < frames; ++f) {
    const unsigned char* s = src + (size_t)f * h * rb;
    unsigned char* d = dst + (size_t)f * h * rb;
    for (int y = 0; y < h; ++y)
      for (int b = 0; b < rb; ++b) h16[(size_t)y * rb + b] = (uint16_t)blur_h_byte(s + (size_t)y * rb, b, w, C, R, tap);
    for (int y = 0; y < h; ++y)
      for (int b = 0; b < rb; ++b) {
        uint32_t V = 0;
        for (int j = -R; j <= R; ++j) V = blur_mac(V, (uint32_t)tap(j < 0 ? -j : j), h16[(size_t)blur_clamp(y + j, h) * rb + b]);
        d[(size_t)y * rb + b] = (unsigned char)blur_round_v(V);
      }
  }
  return true;
}
