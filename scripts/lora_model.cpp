// The addressing of vsd_lora_fuse (videosd_amd/csrc/lora.hip) run on the CPU, on buffers of EXACTLY the size the segments need, built with
// the sanitizers: a wrong offset, leading dimension or row map is an error here and not an out-of-bounds access on the device.
// Two things are run over the shapes of tests/lora_cases.py (rows 4 .. 640, K 64 / 72 / 320 / 576, ranks 1 .. 128, 1 .. 4 adapters, row
// offsets, the GEGLU map, folded destinations, both second copies):
//   * the host twin's loop (lora_core.h lora_fuse_host, what vsd_lora_fuse_host calls) against an element-by-element evaluation of the
//     contract written here with libm's fmaf and explicit partial sums, byte for byte, canaries outside the written bytes intact;
//   * the kernel's own walk -- LORA_BLOCKS_X workgroups striding over tiles of LORA_ROWS rows, a wave's LORA_ROWS_PER_WAVE rows clamped to
//     the last row, K in passes of LORA_KPASS columns, `down` staged LORA_RSTEP ranks at a time, up[row][j0 + lane] -- lane by lane: every
//     read lies inside its buffer, every (row, chunk) of a segment is stored exactly once, at the address the twin writes.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/lora_model.cpp -o /tmp/lora_model && /tmp/lora_model
//
// Exit status 0 and "lora_model: N cases ok" = clean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../videosd_amd/csrc/lora_core.h"

namespace {

constexpr uint16_t CANARY = 0x5A5A;

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  float val(float scale) { return ((int)(next() % 2001) - 1000) * 0.001f * scale; }
};

struct Shape {
  int rows, k, kp, n_dst, row0, map;
  bool fold, bias;
  int copy;
  int n, rank[4], slot[4];
  float alpha[4];
  float scales[4];
};

// heap buffers of exactly the size asked for: the sanitizer guards both ends
template <class T>
struct Buf {
  std::unique_ptr<T[]> p;
  size_t n = 0;
  void make(size_t count) {
    p.reset(new T[count]);
    n = count;
  }
  T* get() const { return p.get(); }
};

struct Data {
  Buf<uint16_t> w0, dst, copy, up[4], down[4];
  Buf<float> gamma, beta, bias, ln_s, ln_t;
  vsd_lora_seg seg;
};

void build(const Shape& s, Rng& rng, Data& d) {
  d.w0.make((size_t)s.rows * s.k);
  for (size_t i = 0; i < d.w0.n; ++i) d.w0.get()[i] = mix_f2h(rng.val(0.1f));
  d.dst.make((size_t)s.n_dst * s.kp);
  std::fill(d.dst.get(), d.dst.get() + d.dst.n, CANARY);
  vsd_lora_seg g;
  memset(&g, 0, sizeof g);
  g.w0 = d.w0.get();
  g.dst = d.dst.get();
  g.rows = s.rows, g.k = s.k, g.kp = s.kp, g.row0 = s.row0, g.map = s.map, g.n = s.n, g.copy_kind = s.copy;
  for (int i = 0; i < s.n; ++i) {
    d.up[i].make((size_t)s.rows * s.rank[i]);
    d.down[i].make((size_t)s.rank[i] * s.k);
    for (size_t j = 0; j < d.up[i].n; ++j) d.up[i].get()[j] = mix_f2h(rng.val(0.2f));
    for (size_t j = 0; j < d.down[i].n; ++j) d.down[i].get()[j] = mix_f2h(rng.val(0.2f));
    g.up[i] = d.up[i].get(), g.down[i] = d.down[i].get(), g.rank[i] = s.rank[i], g.slot[i] = s.slot[i], g.a[i] = s.alpha[i] / (float)s.rank[i];
  }
  if (s.fold) {
    d.gamma.make(s.k), d.beta.make(s.k), d.ln_s.make(s.n_dst), d.ln_t.make(s.n_dst);
    for (int k = 0; k < s.k; ++k) d.gamma.get()[k] = 1.0f + rng.val(0.1f), d.beta.get()[k] = rng.val(0.1f);
    for (int r = 0; r < s.n_dst; ++r) d.ln_s.get()[r] = 1234.5f, d.ln_t.get()[r] = -4321.5f;
    g.gamma = d.gamma.get(), g.beta = d.beta.get(), g.ln_s = d.ln_s.get(), g.ln_t = d.ln_t.get();
    if (s.bias) {
      d.bias.make(s.rows);
      for (int r = 0; r < s.rows; ++r) d.bias.get()[r] = rng.val(0.1f);
      g.bias = d.bias.get();
    }
  }
  if (s.copy != VSD_LORA_COPY_NONE) {
    d.copy.make(s.copy == VSD_LORA_COPY_RAW ? (size_t)s.rows * s.k : (size_t)s.n_dst * s.k);
    std::fill(d.copy.get(), d.copy.get() + d.copy.n, CANARY);
    g.copy = d.copy.get();
  }
  d.seg = g;
}

int fail(const char* what, long long a = 0, long long b = 0, long long c = 0) {
  fprintf(stderr, "lora_model: FAILED: %s (%lld, %lld, %lld)\n", what, a, b, c);
  return 1;
}

// the contract, element by element; what every destination must hold afterwards, into `want` copies
int reference(const Shape& s, const Data& d, std::vector<uint16_t>& dst, std::vector<uint16_t>& copy, std::vector<float>& ln_s, std::vector<float>& ln_t) {
  for (int row = 0; row < s.rows; ++row) {
    int dr;
    if (s.map == VSD_LORA_MAP_GEGLU) {
      const int f = s.rows / 2, r = row < f ? row : row - f;
      dr = s.row0 + 128 * (r / 64) + (row < f ? 0 : 64) + r % 64;
    } else {
      dr = s.row0 + row;
    }
    if (dr < 0 || dr >= s.n_dst) return fail("the reference's destination row lies outside", row, dr);
    volatile float ps[64], pt[64];
    for (int l = 0; l < 64; ++l) ps[l] = pt[l] = 0.0f;
    for (int k = 0; k < s.k; ++k) {
      volatile float acc = mix_h2f(d.w0.get()[(size_t)row * s.k + k]);
      for (int i = 0; i < s.n; ++i) {
        const float sc = s.scales[s.slot[i]];
        if (sc == 0.0f) continue;
        float dd = 0.0f;
        for (int j = 0; j < s.rank[i]; ++j)
          dd = fmaf(mix_h2f(d.up[i].get()[(size_t)row * s.rank[i] + j]), mix_h2f(d.down[i].get()[(size_t)j * s.k + k]), dd);
        volatile float sa = sc * d.seg.a[i];
        volatile float t = sa * dd;
        acc = acc + t;
      }
      const uint16_t wf = mix_f2h(acc);
      uint16_t out = wf;
      if (s.fold) {
        volatile float wg = mix_h2f(wf) * d.gamma.get()[k];
        out = mix_f2h(wg);
        const int l = (k / 8) % 64;
        ps[l] = ps[l] + mix_h2f(out);
        volatile float wb = mix_h2f(wf) * d.beta.get()[k];
        pt[l] = pt[l] + wb;
      }
      dst[(size_t)dr * s.kp + k] = out;
      if (s.copy == VSD_LORA_COPY_RAW) copy[(size_t)row * s.k + k] = wf;
      if (s.copy == VSD_LORA_COPY_FRAG) {
        const size_t o = (((((size_t)dr / 16) * (s.k / 32) + k / 32) * 4 + (k % 32) / 8) * 16 + dr % 16) * 8 + k % 8;
        if (o >= copy.size()) return fail("the reference's fragment address lies outside", dr, k);
        copy[o] = out;
      }
    }
    if (s.fold) {
      for (int h = 32; h >= 1; h /= 2)
        for (int l = 0; l < h; ++l) ps[l] = ps[l] + ps[l + h], pt[l] = pt[l] + pt[l + h];
      ln_s[dr] = ps[0];
      volatile float t = pt[0];
      if (s.bias) t = t + d.bias.get()[row];
      ln_t[dr] = t;
    }
  }
  return 0;
}

// the kernel's walk: every index it forms, checked against the buffers' sizes; every (row, chunk) stored once
int walk(const Shape& s, const Data& d) {
  const vsd_lora_seg& g = d.seg;
  const int rows = s.rows, K = s.k;
  const int ntiles = (rows + LORA_ROWS - 1) / LORA_ROWS;
  std::vector<unsigned char> stored((size_t)rows * (K / LORA_CHUNK), 0);
  for (int bx = 0; bx < LORA_BLOCKS_X; ++bx)
    for (int tile = bx; tile < ntiles; tile += LORA_BLOCKS_X)
      for (int k0 = 0; k0 < K; k0 += LORA_KPASS) {
        for (int i = 0; i < s.n; ++i) {
          const int r = s.rank[i];
          for (int j0 = 0; j0 < r; j0 += LORA_RSTEP) {
            const int jn = std::min(LORA_RSTEP, r - j0);
            for (int t = 0; t < LORA_RSTEP * LORA_LANES; ++t) {  // the staging loop, all 256 threads' turns
              const int jr = t >> 6, c = t & 63, kk = k0 + c * LORA_CHUNK;
              if (jr < jn && kk < K) {
                const size_t o = (size_t)(j0 + jr) * K + kk;
                if (o + 8 > d.down[i].n) return fail("a staged read of down outside the matrix", i, j0 + jr, kk);
                if ((size_t)jr * LORA_KPASS + c * LORA_CHUNK + 8 > (size_t)LORA_RSTEP * LORA_KPASS) return fail("a staged write outside the LDS tile", jr, c);
              }
            }
            for (int wave = 0; wave < LORA_WAVES; ++wave)
              for (int lane = 0; lane < LORA_LANES; ++lane)
                for (int q = 0; q < LORA_ROWS_PER_WAVE; ++q) {
                  const int row = std::min(tile * LORA_ROWS + wave * LORA_ROWS_PER_WAVE + q, rows - 1);
                  if (lane < jn && (size_t)row * r + j0 + lane >= d.up[i].n) return fail("a read of up outside the matrix", i, row, j0 + lane);
                  if ((size_t)(jn - 1) * LORA_KPASS + lane * LORA_CHUNK + 8 > (size_t)LORA_RSTEP * LORA_KPASS) return fail("an LDS read outside the tile", jn, lane);
                }
          }
        }
        for (int wave = 0; wave < LORA_WAVES; ++wave)
          for (int lane = 0; lane < LORA_LANES; ++lane) {
            const int k = k0 + lane * LORA_CHUNK;
            if (k >= K) continue;
            if (s.fold && (size_t)k + 8 > d.gamma.n) return fail("gamma / beta read outside", k);
            for (int q = 0; q < LORA_ROWS_PER_WAVE; ++q) {
              const int rb = tile * LORA_ROWS + wave * LORA_ROWS_PER_WAVE + q, row = std::min(rb, rows - 1);
              if ((size_t)row * K + k + 8 > d.w0.n) return fail("a read of W0 outside the matrix", row, k);
              if (rb >= rows) continue;
              const int64_t dr = g.row0 + lora_map_row(g.map, rows, row);
              if (dr < 0 || (size_t)dr * s.kp + k + 8 > d.dst.n) return fail("a store outside the destination", row, dr, k);
              if (s.copy == VSD_LORA_COPY_RAW && (size_t)row * K + k + 8 > d.copy.n) return fail("a raw-copy store outside", row, k);
              if (s.copy == VSD_LORA_COPY_FRAG && ((size_t)lora_frag_off(dr, k, K) + 8 > d.copy.n || lora_frag_off(dr, k, K) < 0))
                return fail("a fragment-major store outside", dr, k);
              if (s.fold && (size_t)dr >= d.ln_s.n) return fail("a fold vector store outside", dr);
              if (stored[(size_t)row * (K / LORA_CHUNK) + k / LORA_CHUNK]++) return fail("a chunk stored twice", row, k);
            }
          }
      }
  for (size_t i = 0; i < stored.size(); ++i)
    if (!stored[i]) return fail("a chunk never stored", (long long)i);
  return 0;
}

}  // namespace

int main() {
  const Shape shapes[] = {
      {4, 72, 128, 4, 0, 0, false, false, 0, 1, {4}, {0}, {4.0f}, {0.8f}},
      {24, 72, 128, 24, 0, 0, false, false, 0, 1, {12}, {0}, {6.0f}, {1.0f}},
      {64, 64, 64, 64, 0, 0, false, false, 0, 1, {1}, {0}, {1.0f}, {-0.75f}},
      {320, 320, 320, 320, 0, 0, false, false, VSD_LORA_COPY_FRAG, 4, {1, 4, 12, 128}, {0, 1, 2, 3}, {1.0f, 8.0f, 12.0f, 64.0f}, {0.5f, -0.25f, 0.0f, 1.25f}},
      {24, 64, 64, 88, 40, 0, false, false, 0, 2, {4, 12}, {1, 3}, {2.0f, 12.0f}, {9.0f, 0.6f, 9.0f, -1.5f}},
      {256, 64, 64, 256, 0, VSD_LORA_MAP_GEGLU, true, true, 0, 1, {4}, {0}, {4.0f}, {0.7f}},
      {24, 576, 576, 48, 24, 0, true, true, 0, 3, {40, 4, 1}, {0, 1, 2}, {20.0f, 4.0f, 3.0f}, {0.3f, 1.0f, -2.0f}},
      {64, 64, 64, 64, 0, 0, true, false, VSD_LORA_COPY_RAW, 1, {4}, {0}, {1.0f}, {1.0f}},
      {320, 320, 320, 320, 0, 0, true, false, VSD_LORA_COPY_FRAG, 1, {4}, {0}, {4.0f}, {0.8f}},
      {24, 72, 128, 24, 0, 0, false, false, 0, 2, {4, 12}, {0, 2}, {4.0f, 1.0f}, {0.0f, 5.0f, 0.0f, 0.0f}},
      {640, 64, 64, 640, 0, 0, false, false, 0, 1, {4}, {0}, {4.0f}, {1.0f}},
      {24, 320, 320, 24, 0, 0, false, false, 0, 1, {128}, {0}, {128.0f}, {1.0f}},
      {17, 1032, 1088, 17, 0, 0, true, true, 0, 1, {33}, {3}, {33.0f}, {0.0f, 0.0f, 0.0f, 0.5f}},
  };
  Rng rng{777};
  int cases = 0;
  for (const Shape& s : shapes) {
    Data d;
    build(s, rng, d);
    if (const char* why = lora_check_segment(d.seg)) return fail(why, cases);
    if (walk(s, d)) return 1;
    std::vector<uint16_t> dst(d.dst.get(), d.dst.get() + d.dst.n), copy(d.copy.get(), d.copy.get() + d.copy.n);
    std::vector<float> ln_s(d.ln_s.get(), d.ln_s.get() + d.ln_s.n), ln_t(d.ln_t.get(), d.ln_t.get() + d.ln_t.n);
    if (reference(s, d, dst, copy, ln_s, ln_t)) return 1;
    const char* why = nullptr;
    int bad = -1;
    if (lora_fuse_host(&d.seg, 1, s.scales, &why, &bad) != VSD_OK) return fail(why ? why : "the twin refused a good segment", cases, bad);
    if (memcmp(dst.data(), d.dst.get(), dst.size() * 2)) return fail("dst: the twin and the element-by-element contract differ", cases);
    if (copy.size() && memcmp(copy.data(), d.copy.get(), copy.size() * 2)) return fail("copy: the twin and the contract differ", cases);
    if (ln_s.size() && (memcmp(ln_s.data(), d.ln_s.get(), ln_s.size() * 4) || memcmp(ln_t.data(), d.ln_t.get(), ln_t.size() * 4)))
      return fail("ln_s / ln_t: the twin and the contract differ", cases);
    for (int r = 0; r < s.n_dst; ++r)  // the pad columns keep the canary, in every row
      for (int k = s.k; k < s.kp; ++k)
        if (d.dst.get()[(size_t)r * s.kp + k] != CANARY) return fail("a pad column changed", cases, r, k);
    // refused, and nothing written
    vsd_lora_seg g = d.seg;
    g.k = s.k + 4;
    std::vector<uint16_t> before(d.dst.get(), d.dst.get() + d.dst.n);
    if (lora_fuse_host(&g, 1, s.scales, &why, &bad) != VSD_ERR_ARG || bad != 0) return fail("K % 8 != 0 accepted", cases);
    g = d.seg;
    g.rank[0] = VSD_LORA_MAX_RANK + 1;
    if (lora_fuse_host(&g, 1, s.scales, &why, &bad) != VSD_ERR_ARG) return fail("rank 129 accepted", cases);
    float nanscale[4] = {NAN, 0, 0, 0};
    if (lora_fuse_host(&d.seg, 1, nanscale, &why, &bad) != VSD_ERR_ARG) return fail("a NaN scale accepted", cases);
    if (memcmp(before.data(), d.dst.get(), before.size() * 2)) return fail("a refused call wrote", cases);
    ++cases;
  }
  // the GEGLU map is a permutation of the rows, the one pack_geglu builds
  for (int rows : {128, 256, 640}) {
    std::vector<int> seen(rows, 0);
    for (int r = 0; r < rows; ++r) {
      const int64_t m = lora_map_row(VSD_LORA_MAP_GEGLU, rows, r);
      if (m < 0 || m >= rows || seen[(size_t)m]++) return fail("the GEGLU map is no permutation", rows, r, m);
      const bool gate = r >= rows / 2;
      if ((m % 128 >= 64) != gate) return fail("a gate row outside the second half of its tile", rows, r, m);
    }
  }
  printf("lora_model: %d cases ok\n", cases);
  return 0;
}
