// THE ADAPTER FUSE of include/vsd.h in executable form: the element arithmetic, the row map and the fragment-major address, the order of the
// LayerNorm-fold sums, the checks of a segment, and the host loop behind vsd_lora_fuse_host.  Shared by csrc/lora.hip (kernel and host
// twin) and scripts/lora_model.cpp (the host model built with the sanitizers), so that the three cannot drift apart.  Plain C++ but for
// LORA_HD; no HIP headers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vsd.h"
#include "prompt_mix_core.h"  // mix_h2f / mix_f2h: fp16 <-> fp32 by bits, what the device's conversions do

#if defined(__HIPCC__)
#define LORA_HD __host__ __device__ __forceinline__
#else
#define LORA_HD inline
#endif

// Every fp32 operation of the contract is written out and rounds on its own (prompt_mix_core.h has switched contraction off for the
// translation unit; once more for a reader of this file alone).
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

constexpr int LORA_LANES = 64;   // partials of a row sum = lanes of the wave that owns the row
constexpr int LORA_CHUNK = 8;    // halfs per 16-byte chunk
// the kernel's shape (csrc/lora.hip), here so that the host model walks the same tiles
constexpr int LORA_THREADS = 256, LORA_WAVES = 4, LORA_ROWS_PER_WAVE = 4, LORA_ROWS = LORA_WAVES * LORA_ROWS_PER_WAVE;
constexpr int LORA_KPASS = LORA_LANES * LORA_CHUNK;  // columns a wave covers per pass
constexpr int LORA_RSTEP = 32;                       // ranks of a `down` tile staged at once
constexpr int LORA_BLOCKS_X = 32;

// one rank step; the product of two fp16 values is exact in fp32, so this fma IS the contract's multiply and add
LORA_HD float lora_rank_step(float d, float up, float down) { return __builtin_fmaf(up, down, d); }
// acc = fadd(acc, fmul(sa, d)), sa = fmul(s, a)
LORA_HD float lora_add(float acc, float sa, float d) {
  const float t = sa * d;
  return acc + t;
}
LORA_HD float lora_sa(float s, float a) { return s * a; }

// destination row of source row `row` (before row0)
LORA_HD int64_t lora_map_row(int map, int64_t rows, int64_t row) {
  if (map != VSD_LORA_MAP_GEGLU) return row;
  const int64_t f = rows >> 1;
  const int64_t r = row < f ? row : row - f;
  return 128 * (r >> 6) + (row < f ? 0 : 64) + (r & 63);
}

// half offset of the 16-byte chunk (dr, k .. k+7), k % 8 == 0, in the fragment-major layout of pack_mfma_frag over [N][K]
LORA_HD int64_t lora_frag_off(int64_t dr, int64_t k, int64_t K) {
  return ((((dr >> 4) * (K >> 5) + (k >> 5)) * 4 + ((k & 31) >> 3)) * 16 + (dr & 15)) * 8;
}

// ---- the check of one segment: nullptr = fine, else the reason
inline const char* lora_check_segment(const vsd_lora_seg& g) {
  auto mis = [](const void* p, uintptr_t a) { return !p || ((uintptr_t)p & (a - 1)); };
  if (mis(g.w0, 16) || mis(g.dst, 16)) return "w0 / dst null or not 16-byte aligned";
  if (g.rows < 1 || g.rows > (1 << 24)) return "rows outside 1..2^24";
  if (g.k < 8 || g.k > (1 << 20) || (g.k & 7)) return "K outside 8..2^20 or no multiple of 8";
  if (g.kp < g.k || (g.kp & 7) || g.kp > (1 << 21)) return "kp < K or no multiple of 8";
  if (g.row0 < 0 || g.row0 > (1 << 24)) return "row0 outside 0..2^24";
  if (g.n < 1 || g.n > VSD_LORA_MAX) return "n outside 1..4 adapters";
  if (g.reserved != 0) return "reserved must be 0";
  for (int i = 0; i < g.n; ++i) {
    if (mis(g.up[i], 2) || mis(g.down[i], 16)) return "up null or odd / down null or not 16-byte aligned";
    if (g.rank[i] < 1 || g.rank[i] > VSD_LORA_MAX_RANK) return "a rank outside 1..128";
    if (g.slot[i] < 0 || g.slot[i] >= VSD_LORA_MAX || (i > 0 && g.slot[i] <= g.slot[i - 1])) return "slots must increase strictly within 0..3";
    if (!isfinite(g.a[i])) return "an alpha / rank that is not finite";
  }
  if (g.map != VSD_LORA_MAP_ID && g.map != VSD_LORA_MAP_GEGLU) return "map must be VSD_LORA_MAP_ID or VSD_LORA_MAP_GEGLU";
  if (g.map == VSD_LORA_MAP_GEGLU && (g.rows & 127)) return "the GEGLU map needs rows % 128 == 0";
  if (g.gamma || g.beta || g.ln_s || g.ln_t) {
    if (mis(g.gamma, 16) || mis(g.beta, 16) || mis(g.ln_s, 4) || mis(g.ln_t, 4)) return "a folded destination needs gamma, beta (16-byte aligned), ln_s and ln_t";
  }
  if (g.bias && (!g.gamma || ((uintptr_t)g.bias & 3))) return "bias only with a folded destination, 4-byte aligned";
  if (g.copy_kind == VSD_LORA_COPY_NONE) {
    if (g.copy) return "copy without a copy kind";
  } else if (g.copy_kind == VSD_LORA_COPY_RAW || g.copy_kind == VSD_LORA_COPY_FRAG) {
    if (mis(g.copy, 16)) return "copy null or not 16-byte aligned";
    if (g.copy_kind == VSD_LORA_COPY_FRAG && ((g.k & 31) || (g.rows & 15) || (g.row0 & 15))) return "a fragment-major copy needs K % 32 == 0, rows % 16 == 0, row0 % 16 == 0";
  } else {
    return "unknown copy kind";
  }
  return nullptr;
}

inline const char* lora_check_scales(const float* scales) {
  if (!scales) return "scales is null";
  for (int i = 0; i < VSD_LORA_MAX; ++i)
    if (!isfinite(scales[i])) return "a scale is not finite";
  return nullptr;
}

// the fixed tree over the 64 partials
inline float lora_tree_host(float* p) {
  for (int h = LORA_LANES / 2; h >= 1; h >>= 1)
    for (int l = 0; l < h; ++l) p[l] = p[l] + p[l + h];
  return p[0];
}

// ---- the host loop: row by row, chunk by chunk, the contract as written
inline void lora_fuse_segment_host(const vsd_lora_seg& g, const float* scales) {
  const uint16_t* w0 = static_cast<const uint16_t*>(g.w0);
  uint16_t* dst = static_cast<uint16_t*>(g.dst);
  uint16_t* copy = static_cast<uint16_t*>(g.copy);
  float sa[VSD_LORA_MAX];
  bool on[VSD_LORA_MAX];
  for (int i = 0; i < g.n; ++i) {
    const float s = scales[g.slot[i]];
    on[i] = s != 0.0f;
    sa[i] = lora_sa(s, g.a[i]);
  }
  for (int64_t row = 0; row < g.rows; ++row) {
    const int64_t dr = g.row0 + lora_map_row(g.map, g.rows, row);
    float ps[LORA_LANES], pt[LORA_LANES];
    for (int l = 0; l < LORA_LANES; ++l) ps[l] = pt[l] = 0.0f;
    for (int64_t c = 0; c < g.k / LORA_CHUNK; ++c) {
      uint16_t wf[LORA_CHUNK], out[LORA_CHUNK];
      for (int e = 0; e < LORA_CHUNK; ++e) {
        const int64_t k = c * LORA_CHUNK + e;
        float acc = mix_h2f(w0[row * g.k + k]);
        for (int i = 0; i < g.n; ++i) {
          if (!on[i]) continue;
          const uint16_t* up = static_cast<const uint16_t*>(g.up[i]);
          const uint16_t* down = static_cast<const uint16_t*>(g.down[i]);
          float d = 0.0f;
          for (int j = 0; j < g.rank[i]; ++j) d = lora_rank_step(d, mix_h2f(up[row * g.rank[i] + j]), mix_h2f(down[(int64_t)j * g.k + k]));
          acc = lora_add(acc, sa[i], d);
        }
        wf[e] = mix_f2h(acc);
        out[e] = wf[e];
        if (g.gamma) {
          const float w = mix_h2f(wf[e]);
          const float wg = w * g.gamma[k];
          out[e] = mix_f2h(wg);
          const int l = (int)(c % LORA_LANES);
          ps[l] = ps[l] + mix_h2f(out[e]);
          const float wb = w * g.beta[k];
          pt[l] = pt[l] + wb;
        }
      }
      memcpy(dst + dr * g.kp + c * LORA_CHUNK, out, 16);
      if (g.copy_kind == VSD_LORA_COPY_RAW) memcpy(copy + row * g.k + c * LORA_CHUNK, wf, 16);
      if (g.copy_kind == VSD_LORA_COPY_FRAG) memcpy(copy + lora_frag_off(dr, c * LORA_CHUNK, g.k), out, 16);
    }
    if (g.gamma) {
      g.ln_s[dr] = lora_tree_host(ps);
      const float t = lora_tree_host(pt);
      g.ln_t[dr] = g.bias ? t + g.bias[row] : t;
    }
  }
}

// -> VSD_OK, or VSD_ERR_ARG with *why and *bad_seg set; nothing is written before every segment has passed
inline int lora_fuse_host(const vsd_lora_seg* segs, int nseg, const float* scales, const char** why, int* bad_seg) {
  *bad_seg = -1;
  if (!segs || nseg < 1 || nseg > 65535) {
    *why = "1 <= nseg <= 65535 segments";
    return VSD_ERR_ARG;
  }
  if ((*why = lora_check_scales(scales))) return VSD_ERR_ARG;
  for (int i = 0; i < nseg; ++i)
    if ((*why = lora_check_segment(segs[i]))) {
      *bad_seg = i;
      return VSD_ERR_ARG;
    }
  for (int i = 0; i < nseg; ++i) lora_fuse_segment_host(segs[i], scales);
  return VSD_OK;
}
