// The ControlNet merges of one denoising step with a scale PER IMAGE of the launch (include/vsd.h vsd_cn_merge_frames;
// Engine.prepare(frame_options=True)): for every segment j (one of the 13 residuals), image b, row and 8-channel chunk
//     out = fp16(fma(fp32(z), scales[b * scale_stride + col_j], fp32(u)))
// where z is the zero-conv's output (recorded with out_scale = 1 and no residual) and u the UNet tensor it is added to.  The default
// program does this in the zero-convs' epilogue with ONE scale per launch; here the scale depends on the image, which an M tile of the
// GEMM does not know, so it is a pass of its own: ONE launch for all segments of a step.
// Pure streaming (2 reads + 1 write of fp16, ~24 MB per frame and step at SD1.5 512 x 512): blockIdx.z = segment, blockIdx.y = image,
// a grid-stride loop over the image's 16-byte chunks, four independent chunk pairs per lane in flight; consecutive lanes on consecutive
// chunks.  The segment table lives in device memory (the arena's addresses are fixed for the life of a captured program).
#include <stdarg.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CM_THREADS = 256, CM_BLOCKS_X = 32, CM_UNROLL = 4;

__global__ void __launch_bounds__(CM_THREADS) cn_merge_frames_kernel(const vsd_merge_seg* __restrict__ segs, const float* __restrict__ scales,
                                                                    int scale_stride) {
  const vsd_merge_seg sg = segs[blockIdx.z];
  const uint32_t per = (uint32_t)((uint64_t)sg.rows * (uint64_t)sg.channels >> 3);  // 16-byte chunks per image (host check: < 2^31)
  const float sc = scales[(size_t)blockIdx.y * scale_stride + sg.col];
  const size_t base = (size_t)blockIdx.y * per;
  const half8* __restrict__ z = reinterpret_cast<const half8*>(sg.z) + base;
  const half8* __restrict__ u = reinterpret_cast<const half8*>(sg.u) + base;
  half8* __restrict__ o = reinterpret_cast<half8*>(sg.out) + base;
  const uint32_t step = gridDim.x * CM_THREADS;
  for (uint32_t i0 = blockIdx.x * CM_THREADS + threadIdx.x; i0 < per; i0 += step * CM_UNROLL) {
    half8 zv[CM_UNROLL], uv[CM_UNROLL];
#pragma unroll
    for (int k = 0; k < CM_UNROLL; ++k) {
      const uint32_t i = i0 + k * step;
      if (i < per) {
        zv[k] = z[i];
        uv[k] = u[i];
      }
    }
#pragma unroll
    for (int k = 0; k < CM_UNROLL; ++k) {
      const uint32_t i = i0 + k * step;
      if (i < per) {
        half8 y;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          float f = __builtin_fmaf((float)zv[k][c], sc, (float)uv[k][c]);
          asm volatile("" : "+v"(f));  // the fma is rounded to fp32 before it is rounded to fp16: no v_fma_mixlo_f16 (emits nothing)
          y[c] = (half_t)f;
        }
        o[i] = y;
      }
    }
  }
}

}  // namespace

extern "C" int vsd_cn_merge_frames(vsd_ctx* ctx, const vsd_merge_seg* segs_dev, int nseg, const void* scales_dev, int scale_stride, int batch,
                                   void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!segs_dev || ((uintptr_t)segs_dev & 15)) return vsd_fail(ctx, VSD_ERR_ARG, "cn_merge_frames: the segment table must be a 16-byte aligned device pointer");
  if (nseg == 0) {  // forget this table (before its memory is freed or rewritten)
    ctx->merge_tables.erase(segs_dev);
    return VSD_OK;
  }
  if (nseg < 1 || nseg > VSD_MERGE_SEG_MAX) return vsd_fail(ctx, VSD_ERR_ARG, "cn_merge_frames: nseg=%d outside 1..%d", nseg, VSD_MERGE_SEG_MAX);
  if (batch < 1 || batch > 65535) return vsd_fail(ctx, VSD_ERR_ARG, "cn_merge_frames: batch=%d outside 1..65535", batch);
  if (!scales_dev || ((uintptr_t)scales_dev & 3) || scale_stride < 1)
    return vsd_fail(ctx, VSD_ERR_ARG, "cn_merge_frames: scales_dev must be a 4-byte aligned pointer, scale_stride >= 1");
  // a table is read back ONCE (a blocking copy at its first use, the engine's prepare), checked field by field, and trusted from then on:
  // ctx->merge_tables: table -> (segments, largest scale column)
  std::pair<int, int> seen{0, 0};
  auto it = ctx->merge_tables.find(segs_dev);
  if (it != ctx->merge_tables.end()) seen = it->second;
  if (seen.first != nseg) {
    vsd_merge_seg host[VSD_MERGE_SEG_MAX];
    VSD_HIP(ctx, hipMemcpy(host, segs_dev, sizeof(vsd_merge_seg) * (size_t)nseg, hipMemcpyDeviceToHost));
    int64_t maxcol = 0;
    for (int i = 0; i < nseg; ++i) {
      const vsd_merge_seg& g = host[i];
      if (!g.z || !g.u || !g.out || ((g.z | g.u | g.out) & 15))
        return vsd_fail(ctx, VSD_ERR_ARG, "cn_merge_frames: segment %d: z, u and out must be 16-byte aligned addresses", i);
      if (g.channels < 8 || g.channels % 8) return vsd_fail(ctx, VSD_ERR_ARG, "cn_merge_frames: segment %d: channels=%lld is no multiple of 8", i, (long long)g.channels);
      if (g.rows < 1 || g.rows > 0x7fffffffLL || g.channels > 0x7fffffffLL || g.rows * g.channels / 8 > 0x7fffffffLL || g.col < 0 || g.col > 0x7fffffffLL)
        return vsd_fail(ctx, VSD_ERR_ARG, "cn_merge_frames: segment %d: rows=%lld channels=%lld col=%lld", i, (long long)g.rows, (long long)g.channels, (long long)g.col);
      maxcol = g.col > maxcol ? g.col : maxcol;
    }
    seen = {nseg, (int)maxcol};
    ctx->merge_tables[segs_dev] = seen;
  }
  if (seen.second >= scale_stride) return vsd_fail(ctx, VSD_ERR_ARG, "cn_merge_frames: scale column %d with scale_stride=%d", seen.second, scale_stride);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(cn_merge_frames_kernel, dim3(CM_BLOCKS_X, batch, nseg), dim3(CM_THREADS), 0, s, segs_dev, (const float*)scales_dev, scale_stride);
  return ls.finish();
}
