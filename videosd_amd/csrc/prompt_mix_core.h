// THE PROMPT MIX of include/vsd.h in executable form: the element arithmetic, the checks of a segment table and of a call, and the host
// loop behind vsd_prompt_mix_host.  Shared by csrc/prompt_mix.hip (kernel and host twin) and scripts/prompt_mix_model.cpp (the host
// model built with the sanitizers), so that the three cannot drift apart.  Plain C++ but for MIX_HD; no HIP headers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vsd.h"

#if defined(__HIPCC__)
#define MIX_HD __host__ __device__ __forceinline__
#else
#define MIX_HD inline
#endif

// Every fp32 operation of the contract is written out: nothing here is contracted by the compiler, an fma stands where the contract has one.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

// acc = w0 * x0;  acc = fma(wi, xi, acc), i = 1 .. n-1, in component order
template <int N>
MIX_HD float mix_chain(const float* w, const float* x) {
  float acc = w[0] * x[0];
#pragma unroll
  for (int i = 1; i < N; ++i) acc = __builtin_fmaf(w[i], x[i], acc);
  return acc;
}

// Where the 16-byte chunks i0, i0 + step, i0 + 2 step, ... of a segment lie in a destination whose rows are `cpr` chunks long: chunk i is
// (row i / cpr, column i % cpr).  Two integer divisions when the walk starts, none per chunk.  The kernel's lanes walk with this; the
// host model checks it against the divisions.
struct MixWalk {
  uint32_t r, ch, dr, dc, cpr;
  MIX_HD MixWalk(uint32_t i0, uint32_t step, uint32_t cpr_) : r(i0 / cpr_), ch(i0 - (i0 / cpr_) * cpr_), dr(step / cpr_), dc(step - (step / cpr_) * cpr_), cpr(cpr_) {}
  MIX_HD void next() {
    r += dr;
    ch += dc;
    if (ch >= cpr) {
      ch -= cpr;
      r += 1;
    }
  }
};

// fp16 <-> fp32 on the host by bits (round to nearest even, subnormals kept), what the device's conversions do
inline float mix_h2f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 31u, m = h & 0x3ffu, bits;
  if (e == 0) {
    if (m == 0) {
      bits = sign;
    } else {  // subnormal: normalise
      int s = 0;
      while (!(m & 0x400u)) {
        m <<= 1;
        ++s;
      }
      bits = sign | ((uint32_t)(113 - s) << 23) | ((m & 0x3ffu) << 13);
    }
  } else if (e == 31) {
    bits = sign | 0x7f800000u | (m << 13) | (m ? 0x00400000u : 0u);
  } else {
    bits = sign | ((e + 112u) << 23) | (m << 13);
  }
  float f;
  memcpy(&f, &bits, 4);
  return f;
}

inline uint16_t mix_f2h(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? (0x200u | ((x >> 13) & 0x3ffu)) : 0u));
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to infinity (>= 65520)
  if (x < 0x33000001u) return sign;                         // <= 2^-25: rounds to zero (the tie at 2^-25 goes to even = 0)
  const int e = (int)(x >> 23);
  uint32_t m = (x & 0x7fffffu) | 0x800000u;
  int shift;
  uint32_t base;
  if (e < 113) {  // subnormal half: value = m * 2^(e-150), unit 2^-24
    shift = 126 - e;
    base = 0;
  } else {
    shift = 13;
    base = (uint32_t)(e - 112) << 10;
    m &= 0x7fffffu;
  }
  uint32_t q = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (q & 1u))) ++q;  // (a carry out of the mantissa moves into the exponent: the right value)
  return (uint16_t)(sign | (base + q));
}

// ---- checks, shared by vsd_prompt_mix, vsd_prompt_mix_table and vsd_prompt_mix_host: nullptr = fine, else the reason
inline const char* mix_check_segment(const vsd_mix_seg& g, int64_t* frames, bool first) {
  if (g.src_off < 0 || g.dst_off < 0 || g.rows < 1 || g.row_bytes < 16 || g.dst_pitch < g.row_bytes || g.dst_frame_stride < 16 ||
      ((g.src_off | g.dst_off | g.row_bytes | g.dst_pitch | g.dst_frame_stride) & 15) || g.rows > 0x7fffffffLL ||
      g.rows * (g.row_bytes >> 4) > 0x7fffffffLL)
    return "every byte field must be a non-negative multiple of 16, rows >= 1, dst_pitch >= row_bytes";
  if (g.kind != VSD_MIX_F16 && g.kind != VSD_MIX_F32 && g.kind != VSD_MIX_COPY) return "kind must be VSD_MIX_F16, VSD_MIX_F32 or VSD_MIX_COPY";
  if (g.reserved != 0) return "reserved must be 0";
  const int64_t f = g.dst_pitch / g.dst_frame_stride;
  if (f < 1 || g.dst_pitch != f * g.dst_frame_stride || g.dst_frame_stride < g.row_bytes || (!first && f != *frames) || f > 65535)
    return "dst_pitch must be the same whole number (1..65535) of dst_frame_stride in every segment, dst_frame_stride >= row_bytes";
  *frames = f;
  return nullptr;
}

inline const char* mix_check_call(const void* const* src_blocks, const float* weights, int n, const void* dst_block) {
  if (n < 1 || n > VSD_MIX_MAX) return "n must be 1..4 components";
  if (!src_blocks || !weights || !dst_block || ((uintptr_t)dst_block & 15)) return "null or misaligned pointer (blocks are 16-byte aligned)";
  for (int i = 0; i < n; ++i) {
    if (!src_blocks[i] || ((uintptr_t)src_blocks[i] & 15)) return "null or misaligned source block (16-byte aligned)";
    if (!isfinite(weights[i]) || weights[i] < 0.0f) return "a weight is negative or not finite";
  }
  return nullptr;
}

// ---- the host loop: one 16-byte chunk at a time, the addressing of the kernel (chunk i of a segment: row i / cpr, column i % cpr)
template <int N>
inline void mix_chunk_host(const unsigned char* const* src, const float* w, int64_t soff, unsigned char* d, int kind) {
  if (kind == VSD_MIX_COPY || N == 1) {  // (one component: weight 1.0f, the bytes as they are)
    memcpy(d, src[0] + soff, 16);
    return;
  }
  if (kind == VSD_MIX_F16) {
    uint16_t in[N][8], out[8];
    for (int i = 0; i < N; ++i) memcpy(in[i], src[i] + soff, 16);
    for (int e = 0; e < 8; ++e) {
      float x[N];
      for (int i = 0; i < N; ++i) x[i] = mix_h2f(in[i][e]);
      out[e] = mix_f2h(mix_chain<N>(w, x));
    }
    memcpy(d, out, 16);
  } else {
    float in[N][4], out[4];
    for (int i = 0; i < N; ++i) memcpy(in[i], src[i] + soff, 16);
    for (int e = 0; e < 4; ++e) {
      float x[N];
      for (int i = 0; i < N; ++i) x[i] = in[i][e];
      out[e] = mix_chain<N>(w, x);
    }
    memcpy(d, out, 16);
  }
}

template <int N>
inline void mix_host_n(const unsigned char* const* src, const float* w, unsigned char* dst, const vsd_mix_seg* segs, int nseg, int frame) {
  for (int s = 0; s < nseg; ++s) {
    const vsd_mix_seg& g = segs[s];
    const int64_t cpr = g.row_bytes >> 4;
    for (int64_t r = 0; r < g.rows; ++r)
      for (int64_t ch = 0; ch < cpr; ++ch)
        mix_chunk_host<N>(src, w, g.src_off + (r * cpr + ch) * 16, dst + g.dst_off + (int64_t)frame * g.dst_frame_stride + r * g.dst_pitch + ch * 16,
                          (int)g.kind);
  }
}

// -> VSD_OK, or VSD_ERR_ARG with *why set
inline int mix_host(const void* const* src_blocks, const float* weights, int n, void* dst_block, const vsd_mix_seg* segs, int nseg, int frame,
                    const char** why, int* bad_seg) {
  *bad_seg = -1;
  if ((*why = mix_check_call(src_blocks, weights, n, dst_block))) return VSD_ERR_ARG;
  if (!segs || nseg < 1 || nseg > 65535) {
    *why = "1 <= nseg <= 65535 segments";
    return VSD_ERR_ARG;
  }
  int64_t frames = 0;
  for (int i = 0; i < nseg; ++i)
    if ((*why = mix_check_segment(segs[i], &frames, i == 0))) {
      *bad_seg = i;
      return VSD_ERR_ARG;
    }
  if (frame < 0 || frame >= frames) {
    *why = "frame outside the destination's slots";
    return VSD_ERR_ARG;
  }
  const unsigned char* const* src = reinterpret_cast<const unsigned char* const*>(src_blocks);
  unsigned char* dst = static_cast<unsigned char*>(dst_block);
  switch (n) {
    case 1: mix_host_n<1>(src, weights, dst, segs, nseg, frame); break;
    case 2: mix_host_n<2>(src, weights, dst, segs, nseg, frame); break;
    case 3: mix_host_n<3>(src, weights, dst, segs, nseg, frame); break;
    default: mix_host_n<4>(src, weights, dst, segs, nseg, frame); break;
  }
  return VSD_OK;
}
