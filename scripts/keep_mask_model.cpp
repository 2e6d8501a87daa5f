// The device form of the two u8 kernels of the keep mask (videosd_amd/csrc/keep_mask.hip) run on the CPU: the SAME functions the kernels
// loop over (videosd_amd/csrc/keep_mask_core.h) -- mask_wgs / mask_span divide a frame's pixels among workgroups, mask_walk splits a span
// into single pixels, 16-pixel vector steps and single pixels again, mask_block_at places the 8 x 8 block of a latent pixel -- on buffers
// of exactly the operands' size, with all three pointers of the blend at every skew 0..15 of a 16-byte boundary, compared byte for byte
// (bit for bit for the weights) with the host loops behind vsd_mask_blend_host / vsd_mask_latent_host.  Built with the sanitizers, so a
// span past the end of a frame, a vector step that is not inside its span or not aligned on one of its three pointers, a block row outside
// its mask is an error here and not an out-of-bounds access on the device.  Shapes: those of tests/keep_mask_cases.py, and 512 x 512.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/keep_mask_model.cpp -o /tmp/keep_mask_model && /tmp/keep_mask_model
//
// Exit status 0 and "keep_mask_model: N cases ok" = clean.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../videosd_amd/csrc/keep_mask_core.h"

namespace {

struct Rng {  // (any noise will do here: the numpy cases of the tests are not restated)
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

int failures = 0, cases = 0;

#define CHECK(COND_, ...)             \
  do {                                \
    if (!(COND_)) {                   \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                   \
      ++failures;                     \
    }                                 \
  } while (0)

// an operand of n bytes whose first byte lies `skew` bytes past a 16-byte boundary and whose last byte is the last of its allocation
// (exact size: the sanitizer sees one byte too many)
struct Freer {
  void operator()(unsigned char* p) const { free(p); }
};
using Block = std::unique_ptr<unsigned char, Freer>;

unsigned char* place(std::vector<Block>& keep, size_t n, int skew) {
  void* base = nullptr;
  if (posix_memalign(&base, 16, skew + n) != 0) abort();
  keep.emplace_back((unsigned char*)base);
  return (unsigned char*)base + skew;
}

// vsd_mask_blend as the kernel runs it, workgroup by workgroup
void blend_device_form(const unsigned char* src, unsigned char* dst, const unsigned char* mask, int frames, int h, int w, int* vector_steps) {
  const int n = h * w, nwg = mask_wgs(n);
  for (int f = 0; f < frames; ++f) {
    int covered = 0;
    for (int g = 0; g < nwg; ++g) {
      int start, len;
      mask_span(n, nwg, g, start, len);
      CHECK(start >= 0 && len >= 0 && start + len <= n && (len == 0 || start == covered), "span %d of %d over %d pixels: [%d, +%d)", g, nwg, n, start, len);
      covered += len;
      const size_t at = (size_t)f * n + start;
      const unsigned char* m = mask + at;
      const unsigned char* s = src + 3 * at;
      unsigned char* d = dst + 3 * at;
      int head, nvec;
      mask_walk((uintptr_t)m, (uintptr_t)s, (uintptr_t)d, len, head, nvec);
      CHECK(head >= 0 && head <= len && head < 16 && nvec >= 0 && head + MASK_VEC * nvec <= len, "walk of %d pixels: head %d, %d steps", len, head, nvec);
      for (int i = 0; i < head; ++i) mask_blend_pixel(s + 3 * i, d + 3 * i, m[i]);
      for (int i = 0; i < nvec; ++i) {
        const int p = head + i * MASK_VEC;
        CHECK(((((uintptr_t)(m + p)) | ((uintptr_t)(s + 3 * p)) | ((uintptr_t)(d + 3 * p))) & 15) == 0, "vector step at pixel %d is not aligned", p);
        unsigned char mq[16], sq[48], dq[48];  // the step's seven 16-byte words, read whole and written whole as the kernel does
        memcpy(mq, m + p, 16);
        memcpy(sq, s + 3 * p, 48);
        memcpy(dq, d + 3 * p, 48);
        for (int byte = 0; byte < 48; ++byte) dq[byte] = mask_blend_byte(sq[byte], dq[byte], mask_weight(mq[byte / 3]));
        memcpy(d + 3 * p, dq, 48);
        ++*vector_steps;
      }
      for (int i = head + nvec * MASK_VEC; i < len; ++i) mask_blend_pixel(s + 3 * i, d + 3 * i, m[i]);
    }
    CHECK(covered == n, "the spans cover %d of %d pixels", covered, n);
  }
}

// vsd_mask_latent as the kernel runs it, thread by thread: rows as two 4-byte words where the mask is 4-byte aligned
void latent_device_form(const unsigned char* mask, int frames, int h, int w, float* weights) {
  const int lw = w / MASK_BLOCK, lhw = (h / MASK_BLOCK) * lw;
  const bool words = ((uintptr_t)mask & 3) == 0;
  for (int f = 0; f < frames; ++f)
    for (int i = 0; i < lhw; ++i) {
      const int y = i / lw, x = i - y * lw;
      const unsigned char* m = mask + (size_t)f * h * w;
      int S = 0;
      for (int r = 0; r < MASK_BLOCK; ++r) {
        const unsigned char* row = m + mask_block_at(w, y, x, r);
        if (words) {
          CHECK(((uintptr_t)row & 3) == 0, "block row of latent pixel %d is not 4-byte aligned", i);
          uint32_t q[2];
          memcpy(q, row, 8);
          for (int k = 0; k < 2; ++k)
            for (int b = 0; b < 4; ++b) S += mask_weight((int)((q[k] >> (8 * b)) & 255u));
        } else {
          for (int k = 0; k < MASK_BLOCK; ++k) S += mask_weight(row[k]);
        }
      }
      CHECK(S >= 0 && S <= MASK_FULL, "S = %d", S);
      weights[(size_t)f * lhw + i] = mask_latent_weight(S);
    }
}

void fill(unsigned char* p, size_t n, int kind, Rng& rng) {
  static const unsigned char edges[6] = {0, 1, 127, 128, 254, 255};
  for (size_t i = 0; i < n; ++i) p[i] = kind == 0 ? 0 : kind == 1 ? 255 : kind == 2 ? edges[i % 6] : (unsigned char)rng.next();
}

void blend_case(int frames, int h, int w, int skew_s, int skew_d, int skew_m, int kind, Rng& rng, int* vector_steps) {
  const size_t n = (size_t)frames * h * w;
  std::vector<Block> keep;
  unsigned char* src = place(keep, 3 * n, skew_s);
  unsigned char* dst = place(keep, 3 * n, skew_d);
  unsigned char* mask = place(keep, n, skew_m);
  fill(src, 3 * n, 3, rng);
  fill(dst, 3 * n, 3, rng);
  fill(mask, n, kind, rng);
  std::vector<unsigned char> want(dst, dst + 3 * n);
  CHECK(mask_blend_host(src, want.data(), mask, frames, h, w), "the host loop refused %d x %d x %d", frames, h, w);
  blend_device_form(src, dst, mask, frames, h, w, vector_steps);
  CHECK(memcmp(dst, want.data(), 3 * n) == 0, "blend %d x %d x %d at skews %d %d %d, masks %d: bytes differ", frames, h, w, skew_s, skew_d, skew_m, kind);
  if (kind == 0) CHECK(memcmp(dst, src, 3 * n) == 0, "an all-0 mask must give the input");
  ++cases;
}

void latent_case(int frames, int h, int w, int skew, int kind, Rng& rng) {
  const size_t n = (size_t)frames * h * w, lhw = (size_t)frames * (h / 8) * (w / 8);
  std::vector<Block> keep;
  unsigned char* mask = place(keep, n, skew);
  fill(mask, n, kind, rng);
  std::unique_ptr<float[]> got(new float[lhw]), want(new float[lhw]);
  CHECK(mask_latent_host(mask, frames, h, w, want.get()), "the host loop refused %d x %d x %d", frames, h, w);
  latent_device_form(mask, frames, h, w, got.get());
  CHECK(memcmp(got.get(), want.get(), lhw * sizeof(float)) == 0, "latent %d x %d x %d at skew %d, masks %d: bits differ", frames, h, w, skew, kind);
  for (size_t i = 0; i < lhw; ++i) CHECK((kind != 0 || got[i] == 0.0f) && (kind != 1 || got[i] == 1.0f), "weight %g of a constant mask", got[i]);
  ++cases;
}

}  // namespace

int main() {
  Rng rng{2024};
  static const int blend_shapes[][2] = {{1, 1}, {3, 5}, {8, 24}, {16, 40}, {72, 120}, {512, 512}};
  static const int latent_shapes[][2] = {{8, 8}, {16, 24}, {72, 120}, {512, 512}};
  int vector_steps = 0, vector_cases = 0;
  for (auto& hw : blend_shapes)
    for (int frames : {1, 3}) {
      const bool big = hw[0] * hw[1] > 10000;
      for (int ss = 0; ss < 16; ss += big ? 5 : 1)
        for (int sd = 0; sd < 16; sd += big ? 5 : 1)
          for (int sm = 0; sm < 16; sm += big ? 5 : 1) {
            if (!big && hw[0] * hw[1] > 200 && (ss | sd | sm) > 3 && ((ss * 7 + sd * 3 + sm) % 11)) continue;  // (the larger shapes: skews 0..3 in full, a sample beyond)
            const int before = vector_steps;
            blend_case(frames, hw[0], hw[1], ss, sd, sm, (ss + sd + sm) % 4, rng, &vector_steps);
            vector_cases += vector_steps > before;
          }
    }
  CHECK(vector_steps > 0 && vector_cases > 4, "no case took the vector steps");
  for (auto& hw : latent_shapes)
    for (int frames : {1, 3})
      for (int skew = 0; skew < 8; ++skew)
        for (int kind = 0; kind < 4; ++kind) latent_case(frames, hw[0], hw[1], skew, kind, rng);
  CHECK(!mask_latent_args_ok(1, 12, 8) && !mask_latent_args_ok(1, 8, 20) && mask_args_ok(1, 1, 1) && !mask_args_ok(0, 8, 8) && !mask_args_ok(1, 8, MASK_MAX_SIDE + 1),
        "argument checks");
  CHECK(mask_weight(255) == 256 && mask_weight(0) == 0 && mask_weight(128) == 129 && mask_blend_byte(200, 17, 256) == 17 && mask_blend_byte(200, 17, 0) == 200,
        "weight / blend corners");
  if (failures) {
    printf("keep_mask_model: %d FAILURES in %d cases\n", failures, cases);
    return 1;
  }
  printf("keep_mask_model: %d cases ok (%d of them with vector steps, %d steps)\n", cases, vector_cases, vector_steps);
  return 0;
}
