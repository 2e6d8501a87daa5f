// The device form of the colour-match stage (videosd_amd/csrc/color_match.hip) run on the CPU: the SAME functions the three kernels loop over
// (videosd_amd/csrc/color_match_core.h) -- color_wgs / color_span divide a frame among workgroups, color_walk splits a span into scalar
// head, 16-byte vectors and scalar tail, color_match_hist / color_gain / color_match_meanstd / color_blend build a LUT entry -- on buffers
// of exactly the size the library asks for, with frames at every byte offset, compared byte for byte with the host loops behind
// vsd_color_match_host.  Built with the sanitizers, so a span past the end of a frame, a vector access that is not inside its span or not
// aligned, a partial histogram or LUT outside the workspace is an error here and not an out-of-bounds access on the device.  The LUT build
// also runs over the contract's corners: one pixel, one bin, a constant side, the gain cap, Q above 2^32, the largest N.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/color_match_model.cpp -o /tmp/color_match_model && /tmp/color_match_model
//
// Exit status 0 and "color_match_model: N cases ok" = clean.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../videosd_amd/csrc/color_match_core.h"

namespace {

struct Rng {  // (any noise will do here: the numpy cases of the tests are not restated)
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

int failures = 0, cases = 0;

#define CHECK(COND_, ...)          \
  do {                             \
    if (!(COND_)) {                \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                \
      ++failures;                  \
    }                              \
  } while (0)

// the walk of launches 1 and 3 over [p, p + len): every byte exactly once, vectors aligned and inside
template <class Byte, class Vec>
void walk(unsigned char* p, int len, Byte byte, Vec vec) {
  int head, nvec;
  color_walk((uintptr_t)p, len, head, nvec);
  CHECK(head >= 0 && head <= len && head < 16 && nvec >= 0 && head + 16 * nvec <= len && len - head - 16 * nvec < 16, "walk of %d bytes: head %d, %d vectors", len, head, nvec);
  for (int i = 0; i < head; ++i) byte(i);
  for (int i = 0; i < nvec; ++i) {
    const int o = head + (i << 4);
    CHECK((((uintptr_t)(p + o)) & 15) == 0, "vector at offset %d is not aligned", o);
    vec(o);
  }
  for (int i = head + (nvec << 4); i < len; ++i) byte(i);
}

// vsd_color_match as the kernels run it, workgroup by workgroup, into a workspace of exactly vsd_color_match_workspace_bytes
void device_form(const unsigned char* src, unsigned char* dst, int frames, int h, int w, int mode, const int* amounts) {
  const int n = h * w, nbytes = 3 * n, nwg = color_wgs(nbytes);
  const int64_t ws_bytes = color_workspace_bytes(frames, h, w);
  std::unique_ptr<unsigned char[]> ws(new unsigned char[ws_bytes]);  // (exact size: the sanitizer sees one byte too many)
  memset(ws.get(), 0xA5, ws_bytes);
  uint32_t* partial = (uint32_t*)ws.get();
  unsigned char* lut = (unsigned char*)(partial + (size_t)frames * nwg * COLOR_PARTIAL);
  CHECK((int64_t)((lut + (size_t)frames * 768) - ws.get()) <= ws_bytes, "the workspace is too small");
  // launch 1
  for (int f = 0; f < frames; ++f) {
    int covered = 0;
    for (int g = 0; g < nwg; ++g) {
      int start, len;
      color_span(nbytes, nwg, g, start, len);
      CHECK(len == 0 || start == covered, "span %d of %d starts at %d, not at %d", g, nwg, start, covered);
      CHECK(start >= 0 && len >= 0 && start + len <= nbytes, "span %d of %d: [%d, %d) of %d", g, nwg, start, start + len, nbytes);
      covered += len;
      uint32_t* out = partial + ((size_t)f * nwg + g) * COLOR_PARTIAL;
      memset(out, 0, COLOR_PARTIAL * 4);
      for (int side = 0; side < 2; ++side) {
        unsigned char* p = (side ? dst : const_cast<unsigned char*>(src)) + (size_t)f * nbytes + start;
        uint32_t* hist = out + side * 3 * 256;
        walk(
            p, len, [&](int i) { hist[((start + i) % 3) * 256 + p[i]] += 1; },
            [&](int o) {
              int c = (start + o) % 3;
              for (int k = 0; k < 16; ++k) {
                hist[c * 256 + p[o + k]] += 1;
                c = c == 2 ? 0 : c + 1;
              }
            });
      }
    }
    CHECK(covered == nbytes, "the spans cover %d of %d bytes", covered, nbytes);
  }
  // launch 2
  for (int f = 0; f < frames; ++f) {
    uint32_t H[6][256], C[6][256];
    for (int j = 0; j < 6; ++j) {
      uint32_t acc = 0;
      for (int v = 0; v < 256; ++v) {
        uint32_t s = 0;
        for (int g = 0; g < nwg; ++g) s += partial[((size_t)f * nwg + g) * COLOR_PARTIAL + j * 256 + v];
        H[j][v] = s;
        C[j][v] = acc += s;
      }
      CHECK(acc == (uint32_t)n, "histogram %d of frame %d counts %u of %d", j, f, acc, n);
    }
    const int a = color_clamp_amount(amounts[f]);
    for (int c = 0; c < 3; ++c) {
      int64_t mom[4] = {0, 0, 0, 0};
      for (int v = 0; v < 256; ++v) {
        mom[0] += (int64_t)v * H[c][v];
        mom[1] += (int64_t)v * v * H[c][v];
        mom[2] += (int64_t)v * H[3 + c][v];
        mom[3] += (int64_t)v * v * H[3 + c][v];
      }
      const double g = mode == COLOR_MEANSTD ? color_gain(n, mom[0], mom[1], mom[2], mom[3]) : 0.0;
      for (int v = 0; v < 256; ++v) {
        const int m = mode == COLOR_MEANSTD ? color_match_meanstd(n, mom[0], mom[2], g, v) : color_match_hist(C[c], C[3 + c][v], H[3 + c][v]);
        CHECK(m >= 0 && m <= 255, "m(%d) = %d", v, m);
        lut[((size_t)f * 3 + c) * 256 + v] = color_blend(v, m, a);
      }
    }
  }
  // launch 3
  for (int f = 0; f < frames; ++f)
    for (int g = 0; g < nwg; ++g) {
      int start, len;
      color_span(nbytes, nwg, g, start, len);
      const unsigned char* t = lut + (size_t)f * 768;
      unsigned char* p = dst + (size_t)f * nbytes + start;
      walk(
          p, len, [&](int i) { p[i] = t[((start + i) % 3) * 256 + p[i]]; },
          [&](int o) {
            int c = (start + o) % 3;
            for (int k = 0; k < 16; ++k) {
              p[o + k] = t[c * 256 + p[o + k]];
              c = c == 2 ? 0 : c + 1;
            }
          });
    }
}

struct Placed {
  std::unique_ptr<unsigned char[]> buf;
  unsigned char* p;
};

Placed place(size_t total, int skew) {
  for (int k = 0; k < 16; ++k) {  // (allocations are 16-byte aligned: one k fits)
    Placed q;
    const size_t size = total + 16 + k;
    q.buf.reset(new unsigned char[size]);
    q.p = q.buf.get() + size - total;
    if (((uintptr_t)q.p & 15) == (uintptr_t)skew) return q;
  }
  abort();
}

enum Kind { RANDOM, TWO_VALUED, CONST_DST, CONST_SRC, SAME, GAIN_CAP, SRC_255, KINDS };

void fill(Kind kind, Rng& rng, unsigned char* src, unsigned char* dst, int nbytes) {
  for (int i = 0; i < nbytes; ++i) {
    const unsigned char r = (unsigned char)rng.next(), q = (unsigned char)rng.next();
    switch (kind) {
      case RANDOM: src[i] = r, dst[i] = q; break;
      case TWO_VALUED: src[i] = (r & 1) ? 200 : 30, dst[i] = (q % 3) ? 100 : 90; break;
      case CONST_DST: src[i] = r, dst[i] = 77; break;
      case CONST_SRC: src[i] = 200, dst[i] = q; break;
      case SAME: src[i] = dst[i] = r; break;
      case GAIN_CAP: src[i] = r, dst[i] = 128 + (q & 1); break;
      default: src[i] = 255, dst[i] = q; break;
    }
  }
}

void run(int h, int w, int frames, Kind kind, int mode, int skew_src, int skew_dst, Rng& rng) {
  const int nbytes = 3 * h * w;
  const size_t total = (size_t)frames * nbytes;
  // buffers that END with the last frame and whose frames start `skew` bytes past a 16-byte boundary: an access beyond is the sanitizer's
  Placed sbuf = place(total, skew_src), dbuf = place(total, skew_dst);
  unsigned char *s0 = sbuf.p, *d0 = dbuf.p;
  std::vector<unsigned char> src(total), dst(total), want(total);
  fill(kind, rng, src.data(), dst.data(), (int)total);
  std::vector<int> amounts(frames);
  static const int picks[] = {0, 256, 77, 128, 255, 1, 300, -5};
  for (int f = 0; f < frames; ++f) amounts[f] = picks[(f + h + w) % 8];
  want = dst;
  for (int f = 0; f < frames; ++f)
    CHECK(color_match_host(src.data() + (size_t)f * nbytes, want.data() + (size_t)f * nbytes, h, w, mode, color_clamp_amount(amounts[f])), "the host loops refuse %d x %d", w, h);
  memcpy(s0, src.data(), total);
  memcpy(d0, dst.data(), total);
  device_form(s0, d0, frames, h, w, mode, amounts.data());
  CHECK(memcmp(d0, want.data(), total) == 0, "%d x %d, %d frame(s), kind %d, mode %d, skews %d / %d: the device form differs from the host loops", w, h, frames, kind,
        mode, skew_src, skew_dst);
  CHECK(memcmp(s0, src.data(), total) == 0, "src was written");
  if (kind == SAME)
    for (int f = 0; f < frames; ++f)
      if (color_clamp_amount(amounts[f]) == 256)
        CHECK(memcmp(d0 + (size_t)f * nbytes, src.data() + (size_t)f * nbytes, nbytes) == 0, "src == dst did not leave dst as it is (mode %d)", mode);
  ++cases;
}

}  // namespace

int main() {
  Rng rng{20240607};
  static const int shapes[][3] = {{1, 1, 1}, {1, 2, 4}, {1, 5, 3}, {1, 17, 3}, {5, 7, 3}, {8, 8, 1}, {3, 11, 5}, {64, 64, 3}, {72, 120, 5}, {75, 73, 2}, {264, 256, 1}, {2, 16384, 1}, {16384, 1, 1},
                                  {600, 601, 1}};  // (the last: the cap of COLOR_MAX_WGS workgroups, spans that are no multiple of 16 or of 3)
  for (const auto& s : shapes)
    for (int kind = 0; kind < KINDS; ++kind)
      for (int mode = 0; mode < 2; ++mode) {
        const bool small = s[0] * s[1] <= 128;
        for (int skew = 0; skew < (small ? 16 : 3); ++skew) run(s[0], s[1], s[2], (Kind)kind, mode, small ? skew : skew * 5, small ? (skew * 7 + 3) & 15 : skew * 3 + 1, rng);
      }
  // the largest frame: the 64-bit products at their bound (N = 2^23, every src byte 255, dst two-valued at the ends: Vs = 0, Vd maximal)
  {
    const int h = 2048, w = 4096;
    uint32_t H[6][256] = {};
    const int64_t n = (int64_t)h * w;
    for (int c = 0; c < 3; ++c) {
      H[c][255] = (uint32_t)n;
      H[3 + c][0] = (uint32_t)(n / 2);
      H[3 + c][255] = (uint32_t)(n - n / 2);
    }
    unsigned char lut[3][256];
    color_build_lut(H, n, COLOR_MEANSTD, 256, lut);  // (signed overflow in n * q or s * s would stop here)
    CHECK(lut[0][0] == 255 && lut[0][255] == 255, "a constant source at the largest N: %d %d", lut[0][0], lut[0][255]);
    for (int c = 0; c < 3; ++c) {
      memset(H[c], 0, sizeof H[c]);
      H[c][0] = (uint32_t)(n / 2), H[c][255] = (uint32_t)(n - n / 2);
    }
    color_build_lut(H, n, COLOR_MEANSTD, 256, lut);
    CHECK(lut[1][0] == 0 && lut[1][255] == 255 && lut[1][128] == 128, "src == dst at the largest N");
    color_build_lut(H, n, COLOR_HIST, 256, lut);
    CHECK(lut[2][0] == 0 && lut[2][255] == 255, "src == dst at the largest N, histogram mode");
    CHECK(color_workspace_bytes(COLOR_MAX_FRAMES, h, w) > 0 && color_workspace_bytes(1, h, w + 1) == 0 && !color_args_ok(4096, 4096, 0), "the limits");
    ++cases;
  }
  if (failures) {
    printf("color_match_model: %d check(s) failed\n", failures);
    return 1;
  }
  printf("color_match_model: %d cases ok\n", cases);
  return 0;
}
