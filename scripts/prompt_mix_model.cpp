// The addressing of vsd_prompt_mix (videosd_amd/csrc/prompt_mix.hip) run on the CPU, on buffers of EXACTLY the size the segment lists
// need, built with the sanitizers: a wrong offset, pitch or row count is an error here and not an out-of-bounds access on the device.
// Two things are run over awkward segment lists (one-chunk rows, pitched rows, fp32 runs, a copy segment, runs longer than one pass of
// the grid, every frame slot of B = 1, 2, 3, 5; n = 1 .. 4):
//   * the host twin's loop (prompt_mix_core.h mix_host, what vsd_prompt_mix_host calls), against an element-by-element evaluation of the
//     contract written here, byte for byte, with the bytes outside the written rows still the sentinel;
//   * the kernel's own walk -- the grid of MX_BLOCKS_X x 256 lanes, MX_UNROLL chunks per pass, MixWalk stepping without a division --
//     lane by lane: every chunk of a segment is visited exactly once, at the (row, column) the divisions give, inside the buffers.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/prompt_mix_model.cpp -o /tmp/prompt_mix_model && /tmp/prompt_mix_model
//
// Exit status 0 and "prompt_mix_model: N cases ok" = clean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../videosd_amd/csrc/prompt_mix_core.h"

namespace {

constexpr unsigned char SENTINEL = 0xA5;
constexpr int MX_THREADS = 256, MX_BLOCKS_X = 32, MX_UNROLL = 4;  // csrc/prompt_mix.hip

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

struct Case {
  std::vector<vsd_mix_seg> segs;
  int64_t src_bytes = 0, dst_bytes = 0;
  int frames = 1;
};

// one segment after the other, `gap` untouched bytes behind each on both sides
Case make_case(int frames, bool whole) {
  Case c;
  c.frames = whole ? 1 : frames;
  const struct { int64_t rows, rb; int kind; int64_t gap; } items[] = {
      {5, 16, VSD_MIX_F16, 16},  {7, 64, VSD_MIX_F16, 48},  {1, 80, VSD_MIX_F32, 16},          {1, 32, VSD_MIX_COPY, 16}, {3, 16, VSD_MIX_F32, 32},
      {1, 16 * (MX_BLOCKS_X * MX_THREADS * MX_UNROLL + 37), VSD_MIX_F16, 16}, {300, 48, VSD_MIX_F16, 16}, {77, 160, VSD_MIX_F16, 0}};
  for (const auto& it : items) {
    vsd_mix_seg g;
    if (whole) {
      g = {c.src_bytes, c.src_bytes, 1, it.rows * it.rb, it.rows * it.rb, it.rows * it.rb, it.kind, 0};
      c.dst_bytes = c.src_bytes + it.rows * it.rb + it.gap;
    } else {
      g = {c.src_bytes, c.dst_bytes, it.rows, it.rb, frames * it.rb, it.rb, it.kind, 0};
      c.dst_bytes += it.rows * frames * it.rb + it.gap;
    }
    c.src_bytes += it.rows * it.rb + it.gap;
    c.segs.push_back(g);
  }
  if (whole) c.dst_bytes = c.src_bytes;
  return c;
}

// 16-byte aligned heap buffers of exactly `n` bytes (operator new returns 16-byte aligned storage; the sanitizer guards both ends)
std::unique_ptr<unsigned char[]> buffer(int64_t n) { return std::unique_ptr<unsigned char[]>(new unsigned char[(size_t)n]); }

void fill_source(unsigned char* p, const Case& c, Rng& rng) {
  for (int64_t i = 0; i < c.src_bytes; ++i) p[i] = (unsigned char)rng.next();
  for (const auto& g : c.segs) {  // finite values where a segment computes
    if (g.kind == VSD_MIX_COPY) continue;
    const int64_t n = g.rows * g.row_bytes;
    for (int64_t i = 0; i < n; i += g.kind == VSD_MIX_F32 ? 4 : 2) {
      const float v = ((int)(rng.next() % 2001) - 1000) * ldexpf(1.0f, -(int)(rng.next() % 22));
      if (g.kind == VSD_MIX_F32) {
        memcpy(p + g.src_off + i, &v, 4);
      } else {
        const uint16_t h = mix_f2h(v);
        memcpy(p + g.src_off + i, &h, 2);
      }
    }
  }
}

// the contract, element by element, with the plain `fmaf` of libm: no templates, no chunks
void reference(const std::vector<const unsigned char*>& src, const std::vector<float>& w, unsigned char* dst, const Case& c, int frame) {
  const int n = (int)src.size();
  for (const auto& g : c.segs)
    for (int64_t r = 0; r < g.rows; ++r) {
      unsigned char* d = dst + g.dst_off + frame * g.dst_frame_stride + r * g.dst_pitch;
      const int64_t so = g.src_off + r * g.row_bytes;
      if (g.kind == VSD_MIX_COPY || n == 1) {
        memcpy(d, src[0] + so, (size_t)g.row_bytes);
        continue;
      }
      const int es = g.kind == VSD_MIX_F32 ? 4 : 2;
      for (int64_t e = 0; e < g.row_bytes; e += es) {
        float acc = 0.0f;
        for (int i = 0; i < n; ++i) {
          float x;
          if (es == 4) {
            memcpy(&x, src[i] + so + e, 4);
          } else {
            uint16_t h;
            memcpy(&h, src[i] + so + e, 2);
            x = mix_h2f(h);
          }
          volatile float prod = w[i] * x;  // (kept apart from the addition: the first term is a multiply, not an fma with zero)
          acc = i == 0 ? prod : fmaf(w[i], x, acc);
        }
        if (es == 4) {
          memcpy(d + e, &acc, 4);
        } else {
          const uint16_t h = mix_f2h(acc);
          memcpy(d + e, &h, 2);
        }
      }
    }
}

int fail(const char* what, int a = 0, int b = 0, long long c = 0) {
  fprintf(stderr, "prompt_mix_model: FAILED: %s (%d, %d, %lld)\n", what, a, b, c);
  return 1;
}

// the kernel's walk over one segment: which chunks every lane touches, where it reads and where it writes
int walk_segment(const vsd_mix_seg& g, int frame, int64_t src_bytes, int64_t dst_bytes, std::vector<unsigned char>& seen) {
  const uint32_t cpr = (uint32_t)(g.row_bytes >> 4), total = (uint32_t)g.rows * cpr, step = MX_BLOCKS_X * MX_THREADS;
  seen.assign(total, 0);
  for (uint32_t lane = 0; lane < step; ++lane) {
    uint32_t i0 = lane;
    if (i0 >= total) continue;
    MixWalk at(i0, step, cpr);
    for (; i0 < total; i0 += step * MX_UNROLL)
      for (int u = 0; u < MX_UNROLL; ++u) {
        const uint32_t i = i0 + u * step;
        if (i < total) {
          if (at.r != i / cpr || at.ch != i % cpr) return fail("the walk left the chunk's (row, column)", (int)i, (int)at.r, at.ch);
          const int64_t s = g.src_off + (int64_t)i * 16, d = g.dst_off + (int64_t)frame * g.dst_frame_stride + (int64_t)at.r * g.dst_pitch + (int64_t)at.ch * 16;
          if (s < 0 || s + 16 > src_bytes) return fail("a source read outside the block", (int)i, 0, s);
          if (d < 0 || d + 16 > dst_bytes) return fail("a destination write outside the block", (int)i, frame, d);
          if (seen[i]++) return fail("a chunk visited twice", (int)i);
        }
        at.next();
      }
  }
  for (uint32_t i = 0; i < total; ++i)
    if (!seen[i]) return fail("a chunk never visited", (int)i);
  return 0;
}

}  // namespace

int main() {
  int cases = 0;
  Rng rng{12345};
  std::vector<unsigned char> seen;
  const float weights[4][4] = {{1.0f}, {0.25f, 0.75f}, {0.5f, 0.3f, 0.2f}, {0.1f, 0.2f, 0.3f, 0.4f}};
  for (int frames : {1, 2, 3, 5})
    for (int whole = 0; whole < 2; ++whole) {
      if (whole && frames != 1) continue;
      const Case c = make_case(frames, whole != 0);
      for (int f = 0; f < c.frames; ++f)
        for (const auto& g : c.segs)
          if (walk_segment(g, f, c.src_bytes, c.dst_bytes, seen)) return 1;
      for (int n = 1; n <= 4; ++n) {
        std::vector<std::unique_ptr<unsigned char[]>> own;
        std::vector<const unsigned char*> src;
        for (int i = 0; i < n; ++i) {
          own.push_back(buffer(c.src_bytes));
          fill_source(own.back().get(), c, rng);
          src.push_back(own.back().get());
        }
        const std::vector<float> w(weights[n - 1], weights[n - 1] + n);
        for (int f = 0; f < c.frames; ++f) {
          auto got = buffer(c.dst_bytes), want = buffer(c.dst_bytes);
          memset(got.get(), SENTINEL, (size_t)c.dst_bytes);
          memset(want.get(), SENTINEL, (size_t)c.dst_bytes);
          const char* why = nullptr;
          int bad = -1;
          const int rc = mix_host(reinterpret_cast<const void* const*>(src.data()), w.data(), n, got.get(), c.segs.data(), (int)c.segs.size(), f, &why, &bad);
          if (rc != VSD_OK) return fail(why ? why : "mix_host refused a good call", n, f, bad);
          reference(src, w, want.get(), c, f);
          if (memcmp(got.get(), want.get(), (size_t)c.dst_bytes)) return fail("the twin and the element-by-element contract differ", frames, n, f);
          // what was written: the segments' own rows of slot f, nothing else
          std::vector<unsigned char> mine((size_t)c.dst_bytes, 0);
          for (const auto& g : c.segs)
            for (int64_t r = 0; r < g.rows; ++r) memset(mine.data() + g.dst_off + f * g.dst_frame_stride + r * g.dst_pitch, 1, (size_t)g.row_bytes);
          for (int64_t i = 0; i < c.dst_bytes; ++i)
            if (!mine[(size_t)i] && got[(size_t)i] != SENTINEL) return fail("a byte outside the written rows changed", frames, f, i);
          ++cases;
        }
        // refused, and nothing written: a frame the destination does not have, a bad weight, a field that is no multiple of 16
        auto dst = buffer(c.dst_bytes);
        memset(dst.get(), SENTINEL, (size_t)c.dst_bytes);
        const char* why = nullptr;
        int bad = -1;
        const void* const* sp = reinterpret_cast<const void* const*>(src.data());
        if (mix_host(sp, w.data(), n, dst.get(), c.segs.data(), (int)c.segs.size(), c.frames, &why, &bad) != VSD_ERR_ARG) return fail("frame == B accepted");
        std::vector<float> wbad(w);
        wbad[0] = -wbad[0] - 1.0f;
        if (mix_host(sp, wbad.data(), n, dst.get(), c.segs.data(), (int)c.segs.size(), 0, &why, &bad) != VSD_ERR_ARG) return fail("a negative weight accepted");
        wbad[0] = NAN;
        if (mix_host(sp, wbad.data(), n, dst.get(), c.segs.data(), (int)c.segs.size(), 0, &why, &bad) != VSD_ERR_ARG) return fail("a NaN weight accepted");
        std::vector<vsd_mix_seg> off(c.segs);
        off[1].dst_off += 8;
        if (mix_host(sp, w.data(), n, dst.get(), off.data(), (int)off.size(), 0, &why, &bad) != VSD_ERR_ARG || bad != 1) return fail("a misaligned field accepted");
        if (mix_host(sp, w.data(), 0, dst.get(), c.segs.data(), (int)c.segs.size(), 0, &why, &bad) != VSD_ERR_ARG) return fail("n = 0 accepted");
        if (mix_host(sp, w.data(), 5, dst.get(), c.segs.data(), (int)c.segs.size(), 0, &why, &bad) != VSD_ERR_ARG) return fail("n = 5 accepted");
        for (int64_t i = 0; i < c.dst_bytes; ++i)
          if (dst[(size_t)i] != SENTINEL) return fail("a refused call wrote", frames, n, i);
      }
    }
  // the conversions by bits: every fp16 pattern survives the round trip (NaNs keep their class)
  for (uint32_t h = 0; h < 0x10000u; ++h) {
    const float f = mix_h2f((uint16_t)h);
    const uint16_t back = mix_f2h(f);
    const bool nan = (h & 0x7c00u) == 0x7c00u && (h & 0x3ffu);
    if (nan ? !((back & 0x7c00u) == 0x7c00u && (back & 0x3ffu)) : back != h) return fail("fp16 round trip", (int)h, (int)back);
  }
  printf("prompt_mix_model: %d cases ok\n", cases);
  return 0;
}
