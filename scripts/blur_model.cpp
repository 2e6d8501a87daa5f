// c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I videosd_amd/csrc scripts/blur_model.cpp -o /tmp/blur_model && /tmp/blur_model
//
// No GPU.  The kernel of csrc/blur.hip, walked on the CPU: for every tile of every frame the horizontal pass into an image of exactly
// BLUR_LDS_ROWS x BLUR_TILE_W u16, then the vertical pass, slot by slot as the lanes take them, through the SAME blur_tile /
// blur_lds_src_row / blur_group_words / blur_h_group / blur_h_byte / blur_v_byte / blur_round_* of csrc/blur_core.h.  src and dst are
// buffers of exactly frames*C*h*w bytes (what lies ahead of a skewed one is poisoned), every word the window walk reads is checked
// against the operand and for alignment, every image cell is checked to be written before it is read, and every destination byte to be
// written exactly once.  The result is compared with the contract's direct evaluation, the host loops behind vsd_gauss_blur_host.
// Cases: every shape x tap table x channel count of tests/blur_cases.py, src and dst each 16-byte aligned and one byte off, one and three
// frames and the three image contents taking turns.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "blur_core.h"

#if defined(__SANITIZE_ADDRESS__)
#define BLUR_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define BLUR_ASAN 1
#endif
#endif
#if defined(BLUR_ASAN)
#include <sanitizer/asan_interface.h>
#endif

namespace {

int failures = 0, cases = 0;
long word_groups = 0, byte_cells = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (++failures <= 20) {                  \
        printf("FAIL line %d: ", __LINE__);    \
        printf(__VA_ARGS__);                   \
        printf("\n");                          \
      }                                        \
    }                                          \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

struct Block {  // exactly n usable bytes at p; with a skew, the bytes ahead of p are poisoned
  unsigned char* raw;
  unsigned char* p;
  size_t room;
  Block(size_t n, int skew) : room(((n + skew + 15) / 16) * 16) {
    raw = (unsigned char*)aligned_alloc(16, room);
    p = raw + skew;
#if defined(BLUR_ASAN)
    if (skew) __asan_poison_memory_region(raw, skew);
    if (room > n + skew) __asan_poison_memory_region(p + n, room - n - skew);
#endif
  }
  ~Block() {
#if defined(BLUR_ASAN)
    __asan_unpoison_memory_region(raw, room);
#endif
    free(raw);
  }
  Block(const Block&) = delete;
};

struct Taps {
  int32_t t[BLUR_TAPS];
  int operator()(int k) const { return t[1 + k]; }
};

Taps identity() {
  Taps a{};
  a.t[0] = 1;
  a.t[1] = BLUR_ONE;
  return a;
}
Taps gauss(double sigma) {  // the recipe of videosd_amd/blur.py
  Taps a{};
  const int R = (int)fmax(1.0, ceil(3.0 * sigma));
  double g[BLUR_MAX_RADIUS + 1], G = 0;
  for (int i = 0; i <= R; ++i) {
    g[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma));
    G += (i ? 2 : 1) * g[i];
  }
  int rest = BLUR_ONE;
  for (int i = 1; i <= R; ++i) {
    a.t[1 + i] = (int)floor(BLUR_ONE * g[i] / G + 0.5);
    rest -= 2 * a.t[1 + i];
  }
  a.t[0] = R;
  a.t[1] = rest;
  return a;
}
Taps flat32() {
  Taps a{};
  a.t[0] = 32;
  for (int i = 1; i <= 32; ++i) a.t[1 + i] = BLUR_ONE / 65;
  a.t[1] = BLUR_ONE - 64 * (BLUR_ONE / 65);
  return a;
}
Taps far_only(int R) {
  Taps a{};
  a.t[0] = R;
  a.t[1 + R] = BLUR_ONE / 2;
  return a;
}

struct CheckedWord {  // an aligned word of the operand [lo, hi), and nothing else
  uintptr_t lo, hi;
  uint32_t operator()(uintptr_t a) const {
    uint32_t v = 0;
    CHECK((a & 3) == 0, "word address not 4-byte aligned");
    CHECK(a >= lo && a + 4 <= hi, "word at %ld outside the operand of %ld bytes", (long)(a - lo), (long)(hi - lo));
    if ((a & 3) == 0 && a >= lo && a + 4 <= hi) memcpy(&v, (const void*)a, 4);
    return v;
  }
};

void device_form(const unsigned char* src, unsigned char* dst, int frames, int h, int w, int C, const Taps& taps, unsigned char* hits) {
  constexpr int THREADS = 256, GROUPS = BLUR_TILE_W / BLUR_GROUP;
  const bool valid = blur_taps_ok(taps.t);
  const int R = blur_radius(taps.t[0]), rb = C * w;
  const size_t frame = (size_t)h * rb;
  const uintptr_t lo = (uintptr_t)src, hi = lo + (size_t)frames * frame;
  for (int f = 0; f < frames; ++f)
    for (int ty = 0; ty < blur_tiles_y(h); ++ty)
      for (int tx = 0; tx < blur_tiles_x(w, C); ++tx) {
        std::unique_ptr<uint16_t[]> image(new uint16_t[BLUR_LDS_ROWS * BLUR_TILE_W]);  // exactly the kernel's: one row more is an error here
        std::vector<unsigned char> written(BLUR_LDS_ROWS * BLUR_TILE_W, 0);
        const BlurTile t = blur_tile(h, w, C, R, tx, ty);
        CHECK(t.rows <= BLUR_LDS_ROWS && t.c0 < t.c1 && t.c1 - t.c0 <= BLUR_TILE_W && t.y0 < t.y1, "tile (%d, %d)", tx, ty);
        const unsigned char* sf = src + (size_t)f * frame;
        for (int tid = 0; tid < THREADS; ++tid)
          for (int s = tid; s < t.rows * GROUPS; s += THREADS) {
            const int r = s / GROUPS, col = (s - r * GROUPS) * BLUR_GROUP, b = t.c0 + col;
            if (b >= t.c1) continue;
            const unsigned char* row = sf + (size_t)blur_lds_src_row(t, R, r, h) * rb;
            const int at = r * BLUR_TILE_W + col;
            if (blur_group_words(t, b, (uintptr_t)row, lo, hi, R, C)) {
              uint32_t q[BLUR_GROUP];
              CHECK(at % 4 == 0, "an 8-byte image store at cell %d", at);
              blur_h_group((uintptr_t)row, b, C, R, taps, CheckedWord{lo, hi}, q);
              for (int k = 0; k < BLUR_GROUP; ++k) {
                CHECK(!valid || q[k] <= 65280, "h16 = %u", q[k]);
                image[at + k] = (uint16_t)q[k];
                written[at + k] = 1;
              }
              ++word_groups;
            } else {
              for (int k = 0; k < BLUR_GROUP && b + k < t.c1; ++k) {
                image[at + k] = (uint16_t)blur_h_byte(row, b + k, w, C, R, taps);
                written[at + k] = 1;
                ++byte_cells;
              }
            }
          }
        // (the barrier)
        for (int tid = 0; tid < THREADS; ++tid)
          for (int s = tid; s < (t.y1 - t.y0) * GROUPS; s += THREADS) {
            const int yy = s / GROUPS, col = (s - yy * GROUPS) * BLUR_GROUP, b = t.c0 + col;
            if (b >= t.c1) continue;
            const size_t d = (size_t)f * frame + (size_t)(t.y0 + yy) * rb + b;
            for (int k = 0; k < BLUR_GROUP && b + k < t.c1; ++k) {  // (the kernel's group form reads the same cells, four columns at once)
              for (int j = 0; j <= 2 * R; ++j) {
                const int cell = (yy + j) * BLUR_TILE_W + col + k;
                CHECK(cell < BLUR_LDS_ROWS * BLUR_TILE_W && written[cell], "the vertical pass reads image cell %d, which %s", cell,
                      cell < BLUR_LDS_ROWS * BLUR_TILE_W ? "was not written" : "is outside the image");
              }
              dst[d + k] = blur_v_byte(image.get() + yy * BLUR_TILE_W + col + k, BLUR_TILE_W, R, taps);
              ++hits[d + k];
            }
          }
      }
}

void fill(unsigned char* p, int frames, int h, int w, int C, int kind, Rng& rng) {
  const size_t n = (size_t)frames * h * w * C;
  if (kind == 0)
    for (size_t i = 0; i < n; ++i) p[i] = (unsigned char)rng.next();
  else if (kind == 1)
    memset(p, 255, n);
  else {  // a single 255 pixel in each corner
    memset(p, 0, n);
    for (int f = 0; f < frames; ++f)
      for (int y : {0, h - 1})
        for (int x : {0, w - 1})
          for (int c = 0; c < C; ++c) p[(((size_t)f * h + y) * w + x) * C + c] = 255;
  }
}

void blur_case(int frames, int h, int w, int C, int skew_s, int skew_d, const Taps& taps, int kind, Rng& rng) {
  const size_t n = (size_t)frames * h * w * C;
  Block src(n, skew_s), dst(n, skew_d);
  fill(src.p, frames, h, w, C, kind, rng);
  memset(dst.p, 0x5a, n);
  std::vector<unsigned char> want(n), hits(n, 0), before(src.p, src.p + n);
  CHECK(blur_taps_ok(taps.t), "the table of radius %d is not valid", taps.t[0]);
  CHECK(blur_host(src.p, want.data(), frames, h, w, C, taps.t), "the host loops refused %d x %d x %d x %d", frames, h, w, C);
  device_form(src.p, dst.p, frames, h, w, C, taps, hits.data());
  for (size_t i = 0; i < n; ++i) CHECK(hits[i] == 1, "byte %ld of dst written %d times", (long)i, hits[i]);
  CHECK(memcmp(dst.p, want.data(), n) == 0, "%d x %d x %d x %d, R = %d, skews %d %d, content %d: bytes differ", frames, h, w, C, taps.t[0], skew_s, skew_d, kind);
  CHECK(memcmp(src.p, before.data(), n) == 0, "src changed");
  if (kind == 1)
    for (size_t i = 0; i < n; ++i) CHECK(dst.p[i] == 255, "a constant image must stay constant");
  if (taps.t[0] == 1 && taps.t[1] == BLUR_ONE) CHECK(memcmp(dst.p, src.p, n) == 0, "the identity table must return src");
  ++cases;
}

}  // namespace

int main() {
  Rng rng{2025};
  static const int shapes[][2] = {{1, 1},   {1, 70},   {70, 1},
                                  {3, 5},   {31, 33},  {72, 120},
                                  {130, 200}, {BLUR_TILE_H, BLUR_TILE_W}, {BLUR_TILE_H - 1, BLUR_TILE_W - 1}, {BLUR_TILE_H + 1, BLUR_TILE_W + 1}};
  const Taps tables[] = {identity(), gauss(0.5), gauss(1.4), gauss(4.0), gauss(10.0), flat32(), far_only(1), far_only(32)};
  static const int pinned[] = {5, 4668, 3618, 1683, 470, 79, 8, 0};  // gauss(1.4), as tests/test_blur_host.py pins it
  CHECK(memcmp(tables[2].t, pinned, sizeof pinned) == 0, "gauss(1.4)");
  CHECK(tables[1].t[0] == 2 && tables[3].t[0] == 12 && tables[4].t[0] == 30, "radii of 0.5, 4.0, 10.0");
  int turn = 0;
  for (auto& hw : shapes)
    for (const Taps& taps : tables)
      for (int C : {1, 3})
        for (int ss : {0, 1})
          for (int sd : {0, 1}) {
            blur_case(turn % 2 ? 3 : 1, hw[0], hw[1], C, ss, sd, taps, turn % 3, rng);
            ++turn;
          }
  // tables the host check refuses: the walk stays inside its image and the operand all the same (R is clamped), whatever comes out
  {
    Taps bad = flat32();
    bad.t[0] = 1000;
    CHECK(!blur_taps_ok(bad.t), "R = 1000 accepted");
    Block src(3 * 70 * 90 * 3, 1), dst(3 * 70 * 90 * 3, 1);
    std::vector<unsigned char> hits(3 * 70 * 90 * 3, 0);
    fill(src.p, 3, 70, 90, 3, 0, rng);
    device_form(src.p, dst.p, 3, 70, 90, 3, bad, hits.data());
    bad.t[0] = -5;
    bad.t[2] = -77;
    CHECK(!blur_taps_ok(bad.t), "R = -5 accepted");
    memset(hits.data(), 0, hits.size());
    device_form(src.p, dst.p, 3, 70, 90, 3, bad, hits.data());
    cases += 2;
  }
  Taps t = gauss(1.4);
  t.t[1] += 1;
  CHECK(!blur_taps_ok(t.t), "a sum of 16385 accepted");
  t = gauss(1.4);
  t.t[1 + 9] = 1, t.t[1] -= 2;
  CHECK(!blur_taps_ok(t.t), "a tap beyond R accepted");
  CHECK(blur_round_h(255u * BLUR_ONE) == 65280 && blur_round_v(65280u * BLUR_ONE) == 255 && blur_clamp(-3, 5) == 0 && blur_clamp(9, 5) == 4, "corners");
  CHECK(!blur_args_ok(1, 8, 8, 2) && !blur_args_ok(0, 8, 8, 1) && !blur_args_ok(1, 8, BLUR_MAX_SIDE + 1, 1) && blur_args_ok(1024, 1, 1, 3), "argument checks");
  CHECK(word_groups > 0 && byte_cells > 0, "both walks must have been taken");
  if (failures) {
    printf("blur_model: %d FAILURES in %d cases\n", failures, cases);
    return 1;
  }
  printf("blur_model: %d cases ok (%ld groups through words, %ld bytes alone)\n", cases, word_groups, byte_cells);
  return 0;
}
