// Keep masks on the device (include/vsd.h THE KEEP MASK): the pixel blend of the camera frame into the restyled frame behind
// postprocess_rgb, and the per-latent-pixel weights the latent anchor (vsd_latent_keep, csrc/noise.hip) reads.
//
// The weight of a mask byte, the blend of one byte, the division of a frame among workgroups, the walk over a span and the place of a
// latent pixel's 8 x 8 block live in keep_mask_core.h, shared with the host twins and with scripts/keep_mask_model.cpp; the kernels here
// are loops over those.  One launch each, for all frames of the call (blockIdx.y = frame); no LDS, no atomics, no workspace.
// Form: integer elementwise code, memory- and launch-bound.  vsd_mask_blend moves 16 pixels per lane and step where the three pointers
// allow it -- one 16-byte word of the mask, three of either frame -- and single pixels at the ends of a span and wherever they do not.
#include <stdarg.h>  // (common.h's vsd_fail uses va_start and leaves the include to its users)

#include "common.h"
#include "keep_mask_core.h"

static_assert(MASK_MAX_SIDE == VSD_RESAMPLE_MAX_SIDE && MASK_MAX_FRAMES == VSD_MASK_MAX_FRAMES, "one set of limits");

namespace {

constexpr int KM_THREADS = 256;

// grid (mask_wgs(n), frames)
__global__ void __launch_bounds__(KM_THREADS) mask_blend_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                const unsigned char* __restrict__ mask, int n) {
  int start, len;
  mask_span(n, (int)gridDim.x, (int)blockIdx.x, start, len);
  const size_t at = (size_t)blockIdx.y * n + start;
  const unsigned char* m = mask + at;
  const unsigned char* s = src + 3 * at;
  unsigned char* d = dst + 3 * at;
  int head, nvec;
  mask_walk((uintptr_t)m, (uintptr_t)s, (uintptr_t)d, len, head, nvec);
  const int tid = threadIdx.x;
  for (int i = tid; i < head; i += KM_THREADS) mask_blend_pixel(s + 3 * i, d + 3 * i, m[i]);
  for (int i = tid; i < nvec; i += KM_THREADS) {
    const int p = head + i * MASK_VEC;
    const u32x4 mq = *reinterpret_cast<const u32x4*>(m + p);
    const u32x4* sp = reinterpret_cast<const u32x4*>(s + 3 * p);
    u32x4* dp = reinterpret_cast<u32x4*>(d + 3 * p);
    u32x4 sq[3], dq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sq[k] = sp[k];
      dq[k] = dp[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned int word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int byte = 16 * k + 4 * j + b, px = byte / 3;  // (compile-time after unrolling)
          const int a = mask_weight((int)((mq[px >> 2] >> (8 * (px & 3))) & 255u));
          word |= (unsigned int)mask_blend_byte((int)((sq[k][j] >> (8 * b)) & 255u), (int)((dq[k][j] >> (8 * b)) & 255u), a) << (8 * b);
        }
        dq[k][j] = word;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dp[k] = dq[k];
  }
  for (int i = head + nvec * MASK_VEC + tid; i < len; i += KM_THREADS) mask_blend_pixel(s + 3 * i, d + 3 * i, m[i]);
}

__device__ __forceinline__ int km_sum4(unsigned int q) {
  int s = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) s += mask_weight((int)((q >> (8 * b)) & 255u));
  return s;
}

// grid (cdiv(lh * lw, 256), frames): one thread per latent pixel; rows as two 4-byte words where the mask is 4-byte aligned (w is a
// multiple of 8, so then every block row is)
__global__ void __launch_bounds__(KM_THREADS) mask_latent_kernel(const unsigned char* __restrict__ mask, int h, int w, float* __restrict__ weights) {
  const int lw = w / MASK_BLOCK, lhw = (h / MASK_BLOCK) * lw;
  const int i = blockIdx.x * KM_THREADS + threadIdx.x;
  if (i >= lhw) return;
  const int y = i / lw, x = i - y * lw;
  const unsigned char* m = mask + (size_t)blockIdx.y * h * w;
  const bool words = ((uintptr_t)mask & 3) == 0;  // (uniform)
  int S = 0;
#pragma unroll
  for (int r = 0; r < MASK_BLOCK; ++r) {
    const unsigned char* row = m + mask_block_at(w, y, x, r);
    if (words) {
      const unsigned int* q = reinterpret_cast<const unsigned int*>(row);
      S += km_sum4(q[0]) + km_sum4(q[1]);
    } else {
#pragma unroll
      for (int k = 0; k < MASK_BLOCK; ++k) S += mask_weight(row[k]);
    }
  }
  weights[(size_t)blockIdx.y * lhw + i] = mask_latent_weight(S);
}

}  // namespace

extern "C" int vsd_mask_blend_host(const void* src_u8, void* dst_u8, const void* mask_u8, int frames, int h, int w) {
  return mask_blend_host((const unsigned char*)src_u8, (unsigned char*)dst_u8, (const unsigned char*)mask_u8, frames, h, w) ? VSD_OK : VSD_ERR_ARG;
}

extern "C" int vsd_mask_latent_host(const void* mask_u8, int frames, int h, int w, float* weights_f32) {
  return mask_latent_host((const unsigned char*)mask_u8, frames, h, w, weights_f32) ? VSD_OK : VSD_ERR_ARG;
}

extern "C" int vsd_mask_blend(vsd_ctx* ctx, const void* src_u8, void* dst_u8, const void* mask_u8, int frames, int h, int w, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!src_u8 || !dst_u8 || !mask_u8) return vsd_fail(ctx, VSD_ERR_ARG, "mask_blend: null pointer");
  if (!mask_args_ok(frames, h, w))
    return vsd_fail(ctx, VSD_ERR_ARG, "mask_blend: %d frame(s) of %d x %d: frames must be 1..%d, sides 1..%d", frames, w, h, MASK_MAX_FRAMES, MASK_MAX_SIDE);
  hipStream_t s = (hipStream_t)stream;
  const int n = h * w;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(mask_blend_kernel, dim3(mask_wgs(n), frames), dim3(KM_THREADS), 0, s, (const unsigned char*)src_u8, (unsigned char*)dst_u8,
                     (const unsigned char*)mask_u8, n);
  return ls.finish();
}

extern "C" int vsd_mask_latent(vsd_ctx* ctx, const void* mask_u8, int frames, int h, int w, void* weights_f32, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!mask_u8 || !weights_f32 || ((uintptr_t)weights_f32 & 3)) return vsd_fail(ctx, VSD_ERR_ARG, "mask_latent: null pointer, or weights_f32 not 4-byte aligned");
  if (!mask_latent_args_ok(frames, h, w))
    return vsd_fail(ctx, VSD_ERR_ARG, "mask_latent: %d frame(s) of %d x %d: frames must be 1..%d, sides multiples of 8 in 8..%d", frames, w, h,
                    MASK_MAX_FRAMES, MASK_MAX_SIDE);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(mask_latent_kernel, dim3(cdiv((h / MASK_BLOCK) * (w / MASK_BLOCK), KM_THREADS), frames), dim3(KM_THREADS), 0, s,
                     (const unsigned char*)mask_u8, h, w, (float*)weights_f32);
  return ls.finish();
}
