// Colour match on the device (include/vsd.h THE COLOUR CONTRACT): the colour distribution of the input frame onto the output frame, per
// channel, through a 3 x 256 LUT -- by histogram matching or by mean / standard deviation -- blended with the identity by `amount`.
//
// The division of a frame among workgroups, the walk over a span and the arithmetic of a LUT entry live in color_match_core.h, shared
// with the host twin and with scripts/color_match_model.cpp; the kernels here are loops over those.  Three launches per call, always,
// for all frames of the call (blockIdx.y = frame): nothing waits for the host or for another workgroup, there is no global atomic and
// nothing needs zeroing ahead (launch 1 writes every word of the workspace that launch 2 reads, launch 2 every byte launch 3 reads).
// Form: integer elementwise code, memory- and launch-bound.  16-byte vector loads / stores on the aligned middle of a span, single bytes
// at its ends; counts go into wave-private LDS histograms (an LDS atomic meets only lanes of its own wave) and leave the workgroup as
// plain per-lane stores.
#include <stdarg.h>  // (common.h's vsd_fail uses va_start and leaves the include to its users)

#include "color_match_core.h"
#include "common.h"

static_assert(COLOR_MAX_SIDE == VSD_RESAMPLE_MAX_SIDE && COLOR_MAX_PIXELS == VSD_COLOR_MAX_PIXELS && COLOR_MAX_FRAMES == VSD_COLOR_MAX_FRAMES,
              "one set of limits");
static_assert(COLOR_HIST == VSD_COLOR_HIST && COLOR_MEANSTD == VSD_COLOR_MEANSTD, "one set of modes");

namespace {

constexpr int CM_THREADS = 256, CM_WAVES = CM_THREADS / 64;

// count the `len` bytes at p, which lie `o0` bytes into their frame, into h[channel][value] (LDS, this wave's)
__device__ __forceinline__ void cm_count(const unsigned char* __restrict__ p, int o0, int len, unsigned int (*h)[256]) {
  int head, nvec;
  color_walk((uintptr_t)p, len, head, nvec);
  const int tid = threadIdx.x;
  for (int i = tid; i < head; i += CM_THREADS) atomicAdd(&h[(o0 + i) % 3][p[i]], 1u);
  for (int i = tid; i < nvec; i += CM_THREADS) {
    const int o = head + (i << 4);
    const u32x4 q = *reinterpret_cast<const u32x4*>(p + o);
    int c = (o0 + o) % 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        atomicAdd(&h[c][(q[k] >> (8 * b)) & 255u], 1u);
        c = c == 2 ? 0 : c + 1;
      }
    }
  }
  for (int i = head + (nvec << 4) + tid; i < len; i += CM_THREADS) atomicAdd(&h[(o0 + i) % 3][p[i]], 1u);
}

// launch 1.  grid (color_wgs(nbytes), frames); partial: u32 [frames][gridDim.x][6][256]
__global__ void __launch_bounds__(CM_THREADS) color_hist_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ dst, int nbytes,
                                                                unsigned int* __restrict__ partial) {
  __shared__ unsigned int hist[CM_WAVES][6][256];
  const int tid = threadIdx.x, wave = tid >> 6;
  unsigned int* flat = &hist[0][0][0];
  for (int i = tid; i < CM_WAVES * COLOR_PARTIAL; i += CM_THREADS) flat[i] = 0;
  __syncthreads();
  int start, len;
  color_span(nbytes, (int)gridDim.x, (int)blockIdx.x, start, len);
  const size_t at = (size_t)blockIdx.y * nbytes + start;
  cm_count(src + at, start, len, &hist[wave][0]);
  cm_count(dst + at, start, len, &hist[wave][3]);
  __syncthreads();
  unsigned int* out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * COLOR_PARTIAL;
  for (int j = 0; j < 6; ++j) {
    unsigned int s = 0;
    for (int w = 0; w < CM_WAVES; ++w) s += hist[w][j][tid];
    out[j * 256 + tid] = s;
  }
}

__device__ __forceinline__ long long cm_wave_sum(long long x) {
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

// launch 2.  grid (frames), thread v builds entry v of the three channels' LUTs
__global__ void __launch_bounds__(CM_THREADS) color_lut_kernel(const unsigned int* __restrict__ partial, int nwg, int n, int mode,
                                                               const int* __restrict__ amounts, unsigned char* __restrict__ lut) {
  __shared__ unsigned int cum[6][256];            // inclusive prefix sums of the six histograms
  __shared__ unsigned int wave_total[6][CM_WAVES];
  __shared__ long long wave_mom[12][CM_WAVES];    // S and Q of the six histograms, per wave
  const int v = threadIdx.x, lane = v & 63, wave = v >> 6, f = blockIdx.x;
  const unsigned int* p = partial + (size_t)f * nwg * COLOR_PARTIAL;
  // one workgroup walks up to 64 partials: four partials' 24 loads are in flight at a time (one after the other they took 44 us of a
  // 57 us call at 512 x 512)
  unsigned int cnt[6] = {0, 0, 0, 0, 0, 0}, inc[6];
  int g = 0;
  for (; g + 4 <= nwg; g += 4) {
    unsigned int t[4][6];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 6; ++j) t[u][j] = p[(size_t)(g + u) * COLOR_PARTIAL + j * 256 + v];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 6; ++j) cnt[j] += t[u][j];
  }
  for (; g < nwg; ++g)
#pragma unroll
    for (int j = 0; j < 6; ++j) cnt[j] += p[(size_t)g * COLOR_PARTIAL + j * 256 + v];
  for (int j = 0; j < 6; ++j) {
    const unsigned int s = cnt[j];
    unsigned int x = s;  // inclusive scan inside the wave
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned int y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    inc[j] = x;
    if (lane == 63) wave_total[j][wave] = x;
    if (mode == COLOR_MEANSTD) {  // (uniform)
      const long long s1 = cm_wave_sum((long long)v * s), s2 = cm_wave_sum((long long)v * v * s);
      if (lane == 0) {
        wave_mom[2 * j][wave] = s1;
        wave_mom[2 * j + 1][wave] = s2;
      }
    }
  }
  __syncthreads();
  for (int j = 0; j < 6; ++j) {
    unsigned int x = inc[j];
    for (int w = 0; w < wave; ++w) x += wave_total[j][w];
    cum[j][v] = x;
  }
  __syncthreads();
  const int a = color_clamp_amount(amounts[f]);
  for (int c = 0; c < 3; ++c) {
    int m;
    if (mode == COLOR_MEANSTD) {
      long long mom[4];  // ss, qs, sd, qd
      for (int k = 0; k < 4; ++k) {
        const int row = 2 * (c + 3 * (k >> 1)) + (k & 1);
        long long s = 0;
        for (int w = 0; w < CM_WAVES; ++w) s += wave_mom[row][w];
        mom[k] = s;
      }
      const double g = color_gain(n, mom[0], mom[1], mom[2], mom[3]);
      m = color_match_meanstd(n, mom[0], mom[2], g, v);
    } else {
      m = color_match_hist(cum[c], cum[3 + c][v], cnt[3 + c]);
    }
    lut[((size_t)f * 3 + c) * 256 + v] = color_blend(v, m, a);
  }
}

// launch 3.  the grid of launch 1
__global__ void __launch_bounds__(CM_THREADS) color_apply_kernel(unsigned char* __restrict__ dst, int nbytes, const unsigned char* __restrict__ lut) {
  __shared__ unsigned char t[3][256];
  const int tid = threadIdx.x;
  if (tid < 192) reinterpret_cast<unsigned int*>(&t[0][0])[tid] = reinterpret_cast<const unsigned int*>(lut + (size_t)blockIdx.y * 768)[tid];
  __syncthreads();
  int start, len;
  color_span(nbytes, (int)gridDim.x, (int)blockIdx.x, start, len);
  unsigned char* p = dst + (size_t)blockIdx.y * nbytes + start;
  int head, nvec;
  color_walk((uintptr_t)p, len, head, nvec);
  for (int i = tid; i < head; i += CM_THREADS) p[i] = t[(start + i) % 3][p[i]];
  for (int i = tid; i < nvec; i += CM_THREADS) {
    const int o = head + (i << 4);
    u32x4 q = *reinterpret_cast<const u32x4*>(p + o);
    int c = (start + o) % 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned int word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        word |= (unsigned int)t[c][(q[k] >> (8 * b)) & 255u] << (8 * b);
        c = c == 2 ? 0 : c + 1;
      }
      q[k] = word;
    }
    *reinterpret_cast<u32x4*>(p + o) = q;
  }
  for (int i = head + (nvec << 4) + tid; i < len; i += CM_THREADS) p[i] = t[(start + i) % 3][p[i]];
}

}  // namespace

extern "C" int64_t vsd_color_match_workspace_bytes(int frames, int h, int w) { return color_workspace_bytes(frames, h, w); }

extern "C" int vsd_color_match_host(const void* src_u8, void* dst_u8, int h, int w, int mode, int amount) {
  return color_match_host((const unsigned char*)src_u8, (unsigned char*)dst_u8, h, w, mode, amount) ? VSD_OK : VSD_ERR_ARG;
}

extern "C" int vsd_color_match(vsd_ctx* ctx, const void* src_u8, void* dst_u8, int frames, int h, int w, int mode, const void* amounts_dev,
                               void* workspace, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!src_u8 || !dst_u8 || !amounts_dev || !workspace) return vsd_fail(ctx, VSD_ERR_ARG, "color_match: null pointer");
  if (!color_args_ok(h, w, mode) || frames < 1 || frames > COLOR_MAX_FRAMES)
    return vsd_fail(ctx, VSD_ERR_ARG, "color_match: %d frame(s) of %d x %d, mode %d: frames must be 1..%d, sides 1..%d with at most %d pixels, mode %d or %d",
                    frames, w, h, mode, COLOR_MAX_FRAMES, COLOR_MAX_SIDE, COLOR_MAX_PIXELS, COLOR_HIST, COLOR_MEANSTD);
  if (((uintptr_t)workspace & 15) || ((uintptr_t)amounts_dev & 3))
    return vsd_fail(ctx, VSD_ERR_ARG, "color_match: workspace must be 16-byte aligned and amounts_dev 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int n = h * w, nbytes = 3 * n, nwg = color_wgs(nbytes);
  unsigned int* partial = (unsigned int*)workspace;
  unsigned char* lut = (unsigned char*)(partial + (size_t)frames * nwg * COLOR_PARTIAL);
  const dim3 block(CM_THREADS), spans(nwg, frames);
  {
    LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
    hipLaunchKernelGGL(color_hist_kernel, spans, block, 0, s, (const unsigned char*)src_u8, (const unsigned char*)dst_u8, nbytes, partial);
    if (int rc = ls.finish()) return rc;
  }
  {
    LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
    hipLaunchKernelGGL(color_lut_kernel, dim3(frames), block, 0, s, (const unsigned int*)partial, nwg, n, mode, (const int*)amounts_dev, lut);
    if (int rc = ls.finish()) return rc;
  }
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(color_apply_kernel, spans, block, 0, s, (unsigned char*)dst_u8, nbytes, (const unsigned char*)lut);
  return ls.finish();
}
