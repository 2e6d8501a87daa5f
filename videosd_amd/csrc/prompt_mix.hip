// A weighted mix of up to four cached prompts into an engine's own prompt block, or into one frame slot of a per-frame block (include/vsd.h
// THE PROMPT MIX, vsd_prompt_mix; Engine._sync_prompt, blocks.FrameSlots.install).  Every prompt-dependent item of a prompt's constants is
// linear in the text embeddings, so the block of a blend of embeddings is the blend of the blocks: one pass over n sources and one
// destination, (n + 1) x 40 MB at SD1.5 + ControlNet, where the plain prompt takes a device-to-device copy (2 x 40 MB).
// Bandwidth-bound and shaped for that alone: blockIdx.y = the segment, a segment's 16-byte chunks on consecutive lanes (a wave reads 1 KiB
// per source and instruction and writes 1 KiB), MX_UNROLL independent chunks of every source in flight per lane before the first use, no LDS,
// MX_BLOCKS_X x segments workgroups (~4000 at SD1.5 + ControlNet: ~16 per CU to hide HBM latency; the workgroups of a small segment leave
// at once).  The sources and weights are launch arguments: nothing is uploaded.  A pitched destination (V^T columns of a frame slot) is
// walked with two integer divisions per LANE -- where its first chunk lies, and what a grid stride is in (rows, chunks) -- not per chunk.
// The arithmetic and the checks live in prompt_mix_core.h, shared with the host twin below and scripts/prompt_mix_model.cpp.
#include <stdarg.h>

#include "common.h"
#include "prompt_mix_core.h"

namespace {

constexpr int MX_THREADS = 256, MX_BLOCKS_X = 32, MX_UNROLL = 4;

struct MixArgs {
  const unsigned char* src[VSD_MIX_MAX];
  float w[VSD_MIX_MAX];
};

template <int N>
__device__ __forceinline__ u32x4 mix_chunk(const u32x4* v, const float* w, int kind) {
  if (N == 1 || kind == VSD_MIX_COPY) return v[0];
  u32x4 o;
  if (kind == VSD_MIX_F16) {
    half8 in[N], out;
#pragma unroll
    for (int i = 0; i < N; ++i) in[i] = __builtin_bit_cast(half8, v[i]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x[N];
#pragma unroll
      for (int i = 0; i < N; ++i) x[i] = (float)in[i][e];
      out[e] = (half_t)mix_chain<N>(w, x);
    }
    o = __builtin_bit_cast(u32x4, out);
  } else {
    f32x4 in[N], out;
#pragma unroll
    for (int i = 0; i < N; ++i) in[i] = __builtin_bit_cast(f32x4, v[i]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x[N];
#pragma unroll
      for (int i = 0; i < N; ++i) x[i] = in[i][e];
      out[e] = mix_chain<N>(w, x);
    }
    o = __builtin_bit_cast(u32x4, out);
  }
  return o;
}

template <int N>
__global__ void __launch_bounds__(MX_THREADS) prompt_mix_kernel(const MixArgs a, unsigned char* __restrict__ dst, const vsd_mix_seg* __restrict__ segs,
                                                               int frame) {
  const vsd_mix_seg sg = segs[blockIdx.y];
  const uint32_t cpr = (uint32_t)(sg.row_bytes >> 4);  // 16-byte chunks per row
  const uint32_t total = (uint32_t)sg.rows * cpr;      // (checked on the host: below 2^31)
  const uint32_t step = gridDim.x * MX_THREADS;
  uint32_t i0 = blockIdx.x * MX_THREADS + threadIdx.x;
  if (i0 >= total) return;
  const int kind = (int)sg.kind;
  const int ns = (N == 1 || kind == VSD_MIX_COPY) ? 1 : N;  // a copy segment reads component 0 alone
  unsigned char* d = dst + sg.dst_off + (uint64_t)frame * sg.dst_frame_stride;
  // the sources are dense: chunk i at src_off + 16 i.  The destination: chunk i = (row r, column ch); a grid stride is (dr rows, dc chunks)
  MixWalk at(i0, step, cpr);
  float w[N];
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = a.w[i];
  for (; i0 < total; i0 += step * MX_UNROLL) {
    u32x4 v[MX_UNROLL][N];
#pragma unroll
    for (int u = 0; u < MX_UNROLL; ++u) {
      const uint32_t i = i0 + u * step;
      if (i < total) {
#pragma unroll
        for (int c = 0; c < N; ++c)
          if (c < ns) v[u][c] = *reinterpret_cast<const u32x4*>(a.src[c] + sg.src_off + (uint64_t)i * 16);
      }
    }
#pragma unroll
    for (int u = 0; u < MX_UNROLL; ++u) {
      const uint32_t i = i0 + u * step;
      if (i < total) *reinterpret_cast<u32x4*>(d + (uint64_t)at.r * sg.dst_pitch + (uint64_t)at.ch * 16) = mix_chunk<N>(v[u], w, kind);
      at.next();  // (also past the end: the position is only used under i < total)
    }
  }
}

// what the context knows of a table it has seen: (segments, frame slots of its destination); a table is read back ONCE and trusted after
int mix_table(vsd_ctx* ctx, const vsd_mix_seg* segs_dev, int nseg, std::pair<int, int>* seen) {
  if (!segs_dev || ((uintptr_t)segs_dev & 15)) return vsd_fail(ctx, VSD_ERR_ARG, "prompt_mix: the segment table must be a 16-byte aligned device pointer");
  if (nseg < 1 || nseg > 65535) return vsd_fail(ctx, VSD_ERR_ARG, "prompt_mix: %d segments (1..65535)", nseg);
  auto it = ctx->mix_tables.find(segs_dev);
  if (it != ctx->mix_tables.end() && it->second.first == nseg) {
    *seen = it->second;
    return VSD_OK;
  }
  std::vector<vsd_mix_seg> host((size_t)nseg);
  VSD_HIP(ctx, hipMemcpy(host.data(), segs_dev, sizeof(vsd_mix_seg) * (size_t)nseg, hipMemcpyDeviceToHost));
  int64_t frames = 0;
  for (int i = 0; i < nseg; ++i)
    if (const char* why = mix_check_segment(host[i], &frames, i == 0)) return vsd_fail(ctx, VSD_ERR_ARG, "prompt_mix: segment %d: %s", i, why);
  *seen = {nseg, (int)frames};
  ctx->mix_tables[segs_dev] = *seen;
  return VSD_OK;
}

}  // namespace

extern "C" int vsd_prompt_mix_table(vsd_ctx* ctx, const vsd_mix_seg* segs_dev, int nseg) {
  if (!ctx) return VSD_ERR_ARG;
  if (nseg == 0) {  // forget this table (before its memory is freed or rewritten)
    ctx->mix_tables.erase(segs_dev);
    return VSD_OK;
  }
  std::pair<int, int> seen;
  return mix_table(ctx, segs_dev, nseg, &seen);
}

extern "C" int vsd_prompt_mix(vsd_ctx* ctx, const void* const* src_blocks, const float* weights, int n, void* dst_block,
                              const vsd_mix_seg* segs_dev, int nseg, int frame, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (const char* why = mix_check_call(src_blocks, weights, n, dst_block)) return vsd_fail(ctx, VSD_ERR_ARG, "prompt_mix: %s", why);
  std::pair<int, int> seen;
  if (int rc = mix_table(ctx, segs_dev, nseg, &seen)) return rc;
  if (frame < 0 || frame >= seen.second)
    return vsd_fail(ctx, VSD_ERR_ARG, "prompt_mix: frame %d: the destination has slots 0..%d", frame, seen.second - 1);
  MixArgs a;
  for (int i = 0; i < VSD_MIX_MAX; ++i) {
    a.src[i] = (const unsigned char*)src_blocks[i < n ? i : 0];
    a.w[i] = i < n ? weights[i] : 0.0f;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(MX_BLOCKS_X, nseg), block(MX_THREADS);
  unsigned char* dst = (unsigned char*)dst_block;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  switch (n) {
    case 1: hipLaunchKernelGGL(prompt_mix_kernel<1>, grid, block, 0, s, a, dst, segs_dev, frame); break;
    case 2: hipLaunchKernelGGL(prompt_mix_kernel<2>, grid, block, 0, s, a, dst, segs_dev, frame); break;
    case 3: hipLaunchKernelGGL(prompt_mix_kernel<3>, grid, block, 0, s, a, dst, segs_dev, frame); break;
    default: hipLaunchKernelGGL(prompt_mix_kernel<4>, grid, block, 0, s, a, dst, segs_dev, frame); break;
  }
  return ls.finish();
}

extern "C" int vsd_prompt_mix_host(const void* const* src_blocks, const float* weights, int n, void* dst_block, const vsd_mix_seg* segs,
                                   int nseg, int frame) {
  const char* why;
  int bad;
  return mix_host(src_blocks, weights, n, dst_block, segs, nseg, frame, &why, &bad);
}
