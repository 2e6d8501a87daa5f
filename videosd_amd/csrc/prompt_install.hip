// One cached prompt into frame slot `frame` of a per-frame prompt block (include/vsd.h vsd_prompt_install; Engine.prepare(frame_prompts=True)):
// a launch whose frames have prompts of their own reads, per BasicTransformerBlock, K as [B*tl][c] and V^T as [c][B*ldt]; a cache entry holds
// ONE prompt's K [tl][c] and V^T [c][ldt].  Installing it is a strided copy per block and tensor -- a K segment is one run, a V^T segment c
// rows of ldt*2 bytes at pitch B*ldt*2 -- described by a table in device memory that is built once per pair of layouts.
// Pure data movement, ~7 MB per prompt at SD1.5 + ControlNet: one launch, blockIdx.y = the segment, a row's 16-byte chunks on consecutive
// lanes (a wave moves 1 KiB per instruction on both sides), four independent chunks per lane in flight.
#include <stdarg.h>

#include "common.h"

namespace {

constexpr int PI_THREADS = 256, PI_BLOCKS_X = 8, PI_UNROLL = 4;

__global__ void __launch_bounds__(PI_THREADS) prompt_install_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                   const vsd_prompt_seg* __restrict__ segs, int frame) {
  const vsd_prompt_seg sg = segs[blockIdx.y];
  const uint32_t cpr = (uint32_t)(sg.row_bytes >> 4);  // 16-byte chunks per row
  const uint32_t total = (uint32_t)sg.rows * cpr;
  const unsigned char* s = src + sg.src_off;  // (the source rows follow each other: a cache entry's tensors are dense)
  unsigned char* d = dst + sg.dst_off + (uint64_t)frame * sg.dst_frame_stride;
  const uint32_t step = gridDim.x * PI_THREADS;
  for (uint32_t i0 = blockIdx.x * PI_THREADS + threadIdx.x; i0 < total; i0 += step * PI_UNROLL) {
    u32x4 v[PI_UNROLL];
#pragma unroll
    for (int u = 0; u < PI_UNROLL; ++u) {
      const uint32_t i = i0 + u * step;
      if (i < total) v[u] = *reinterpret_cast<const u32x4*>(s + (uint64_t)i * 16);
    }
#pragma unroll
    for (int u = 0; u < PI_UNROLL; ++u) {
      const uint32_t i = i0 + u * step;
      if (i < total) {
        const uint32_t r = i / cpr, ch = i - r * cpr;
        *reinterpret_cast<u32x4*>(d + (uint64_t)r * sg.dst_pitch + (uint64_t)ch * 16) = v[u];
      }
    }
  }
}

}  // namespace

extern "C" int vsd_prompt_install(vsd_ctx* ctx, const void* src_block, void* dst_block, const vsd_prompt_seg* segs_dev, int nseg, int frame,
                                  void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!segs_dev || ((uintptr_t)segs_dev & 15)) return vsd_fail(ctx, VSD_ERR_ARG, "prompt_install: the segment table must be a 16-byte aligned device pointer");
  // What the host knows of a table it has seen (ctx->prompt_tables: table -> (segments, frame slots of its destination)): a table is read
  // back ONCE -- a blocking copy at its first install, the engine's prepare --, checked field by field, and trusted from then on.
  if (nseg == 0) {  // forget this table (before its memory is freed or rewritten)
    ctx->prompt_tables.erase(segs_dev);
    return VSD_OK;
  }
  if (!src_block || !dst_block || ((uintptr_t)src_block & 15) || ((uintptr_t)dst_block & 15) || nseg < 0 || nseg > 65535)
    return vsd_fail(ctx, VSD_ERR_ARG, "prompt_install: bad arguments (blocks 16-byte aligned, 1 <= nseg <= 65535)");
  std::pair<int, int> seen{0, 0};
  auto it = ctx->prompt_tables.find(segs_dev);
  if (it != ctx->prompt_tables.end()) seen = it->second;
  if (seen.first != nseg) {
    std::vector<vsd_prompt_seg> host((size_t)nseg);
    VSD_HIP(ctx, hipMemcpy(host.data(), segs_dev, sizeof(vsd_prompt_seg) * (size_t)nseg, hipMemcpyDeviceToHost));
    int64_t frames = 0;
    for (int i = 0; i < nseg; ++i) {
      const vsd_prompt_seg& g = host[i];
      if (g.src_off < 0 || g.dst_off < 0 || g.rows < 1 || g.row_bytes < 16 || g.dst_pitch < g.row_bytes || g.dst_frame_stride < 16 ||
          ((g.src_off | g.dst_off | g.row_bytes | g.dst_pitch | g.dst_frame_stride) & 15) || g.rows * (g.row_bytes >> 4) > 0x7fffffffLL)
        return vsd_fail(ctx, VSD_ERR_ARG, "prompt_install: segment %d: every byte field must be a non-negative multiple of 16, rows >= 1, "
                        "dst_pitch >= row_bytes", i);
      // the frame slots of a destination row: what dst_pitch holds of dst_frame_stride; the same for every segment
      const int64_t f = g.dst_pitch / g.dst_frame_stride;
      if (f < 1 || g.dst_pitch != f * g.dst_frame_stride || g.dst_frame_stride < g.row_bytes || (i > 0 && f != frames))
        return vsd_fail(ctx, VSD_ERR_ARG, "prompt_install: segment %d: dst_pitch must be the same whole number of dst_frame_stride in every "
                        "segment, dst_frame_stride >= row_bytes", i);
      frames = f;
    }
    if (frames > 65535) return vsd_fail(ctx, VSD_ERR_ARG, "prompt_install: %lld frame slots", (long long)frames);
    seen = {nseg, (int)frames};
    ctx->prompt_tables[segs_dev] = seen;
  }
  if (frame < 0 || frame >= seen.second)
    return vsd_fail(ctx, VSD_ERR_ARG, "prompt_install: frame %d: the destination has slots 0..%d", frame, seen.second - 1);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(prompt_install_kernel, dim3(PI_BLOCKS_X, nseg), dim3(PI_THREADS), 0, s, (const unsigned char*)src_block,
                     (unsigned char*)dst_block, segs_dev, frame);
  return ls.finish();
}
