// LoRA adapters fused into the packed weights on the device (include/vsd.h THE ADAPTER FUSE, vsd_lora_fuse; Engine.set_adapter_scales).
// Wf = fp16(W0 + sum_i s_i a_i up_i down_i) is computed from kept base copies and written straight into the kernel layout the captured
// programs read by address: the packed [N][kp] matrix (plain, LayerNorm-folded with its ln_s / ln_t row sums, GEGLU-tiled), and the
// second copies (raw to_q of an absorbed block, fragment-major weights of the fused tail).  ONE launch over a device table of segments:
// blockIdx.y = the segment, blockIdx.x strides over its tiles of LORA_ROWS rows; the scales are launch arguments.
// Shape: a wave owns LORA_ROWS_PER_WAVE whole rows (so a folded row's two sums are lane partials and one shuffle tree, no atomics) and
// walks K in passes of 64 lanes x 8 halfs -- a 16-byte load of W0 and a 16-byte store per lane and row.  The four waves of a workgroup
// share each [LORA_RSTEP ranks][512 columns] tile of `down`, staged once in LDS (32 KB) and read back as ds_read_b128 on consecutive
// lanes; up[row][j] is uniform in a wave: 32 ranks sit one per lane and are broadcast with v_readlane.  Per lane and rank step: one
// LDS read, 8 conversions, 4 broadcasts, 32 fp32 fmas.  178 VGPRs, 32 KB of LDS, no scratch: two waves per SIMD.
// The arithmetic, the row map, the fragment address and the checks live in lora_core.h, shared with the host twin below and
// scripts/lora_model.cpp.
#include <stdarg.h>

#include "common.h"
#include "lora_core.h"

namespace {

struct LoraScales {
  float s[VSD_LORA_MAX];
};

constexpr int RPW = LORA_ROWS_PER_WAVE;

__device__ __forceinline__ float lane_bcast(float v, int src_lane) {  // src_lane uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src_lane));
}

__global__ void __launch_bounds__(LORA_THREADS) lora_fuse_kernel(const vsd_lora_seg* __restrict__ segs, const LoraScales sc) {
  __shared__ __attribute__((aligned(16))) half_t stage[LORA_RSTEP][LORA_KPASS];
  const vsd_lora_seg* __restrict__ g = segs + blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = (int)g->rows, K = (int)g->k, n = g->n, map = g->map, copy_kind = g->copy_kind;
  const int64_t kp = g->kp, row0 = g->row0;
  const half_t* __restrict__ w0 = static_cast<const half_t*>(g->w0);
  half_t* __restrict__ dst = static_cast<half_t*>(g->dst);
  half_t* __restrict__ copy = static_cast<half_t*>(g->copy);
  const float* __restrict__ gamma = g->gamma;
  const float* __restrict__ beta = g->beta;
  const int ntiles = (rows + LORA_ROWS - 1) / LORA_ROWS;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int rbase = tile * LORA_ROWS + wave * RPW;
    int row[RPW];  // rows past the end are computed on the last row and not stored: no divergence inside the wave, no read out of bounds
#pragma unroll
    for (int q = 0; q < RPW; ++q) row[q] = min(rbase + q, rows - 1);
    float ps[RPW], pt[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) ps[q] = pt[q] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += LORA_KPASS) {
      const int k = k0 + lane * LORA_CHUNK;
      const bool act = k < K;  // (K % 8 == 0: a chunk is inside the row or outside it)
      float acc[RPW][LORA_CHUNK];
#pragma unroll
      for (int q = 0; q < RPW; ++q) {
        half8 w = {0, 0, 0, 0, 0, 0, 0, 0};
        if (act) w = *reinterpret_cast<const half8*>(w0 + (int64_t)row[q] * K + k);
#pragma unroll
        for (int e = 0; e < LORA_CHUNK; ++e) acc[q][e] = (float)w[e];
      }
      for (int i = 0; i < n; ++i) {
        const int slot = g->slot[i];
        const float s = slot == 0 ? sc.s[0] : slot == 1 ? sc.s[1] : slot == 2 ? sc.s[2] : sc.s[3];
        if (s == 0.0f) continue;  // (uniform in the workgroup: the barriers below are met by all or by none)
        const float sa = lora_sa(s, g->a[i]);
        const int r = g->rank[i];
        const half_t* __restrict__ up = static_cast<const half_t*>(g->up[i]);
        const half_t* __restrict__ down = static_cast<const half_t*>(g->down[i]);
        float d[RPW][LORA_CHUNK];
#pragma unroll
        for (int q = 0; q < RPW; ++q)
#pragma unroll
          for (int e = 0; e < LORA_CHUNK; ++e) d[q][e] = 0.0f;
        for (int j0 = 0; j0 < r; j0 += LORA_RSTEP) {
          const int jn = min(LORA_RSTEP, r - j0);
          __syncthreads();  // the tile staged before has been read by every wave
          for (int t = threadIdx.x; t < LORA_RSTEP * LORA_LANES; t += LORA_THREADS) {
            const int jr = t >> 6, c = t & 63, kk = k0 + c * LORA_CHUNK;
            if (jr < jn && kk < K)
              *reinterpret_cast<u32x4*>(&stage[jr][c * LORA_CHUNK]) = *reinterpret_cast<const u32x4*>(down + (int64_t)(j0 + jr) * K + kk);
          }
          float u[RPW];  // up[row][j0 + lane], lanes 0 .. jn-1
#pragma unroll
          for (int q = 0; q < RPW; ++q) u[q] = lane < jn ? (float)up[(int64_t)row[q] * r + j0 + lane] : 0.0f;
          __syncthreads();
          for (int jr = 0; jr < jn; ++jr) {
            const half8 dn = *reinterpret_cast<const half8*>(&stage[jr][lane * LORA_CHUNK]);  // (a lane past K reads what nobody staged and stores nothing)
            float dnf[LORA_CHUNK];
#pragma unroll
            for (int e = 0; e < LORA_CHUNK; ++e) dnf[e] = (float)dn[e];
#pragma unroll
            for (int q = 0; q < RPW; ++q) {
              const float uq = lane_bcast(u[q], jr);
#pragma unroll
              for (int e = 0; e < LORA_CHUNK; ++e) d[q][e] = lora_rank_step(d[q][e], uq, dnf[e]);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < RPW; ++q)
#pragma unroll
          for (int e = 0; e < LORA_CHUNK; ++e) acc[q][e] = lora_add(acc[q][e], sa, d[q][e]);
      }
      if (act) {
        float gm[LORA_CHUNK], bt[LORA_CHUNK];
        if (gamma) {
          const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + k), g1 = *reinterpret_cast<const f32x4*>(gamma + k + 4);
          const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + k), b1 = *reinterpret_cast<const f32x4*>(beta + k + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            gm[e] = g0[e];
            gm[e + 4] = g1[e];
            bt[e] = b0[e];
            bt[e + 4] = b1[e];
          }
        }
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
          if (rbase + q >= rows) continue;
          const int64_t dr = row0 + lora_map_row(map, rows, row[q]);
          half8 wf, out;
#pragma unroll
          for (int e = 0; e < LORA_CHUNK; ++e) wf[e] = (half_t)acc[q][e];
          out = wf;
          if (gamma) {
#pragma unroll
            for (int e = 0; e < LORA_CHUNK; ++e) {
              const float w = (float)wf[e];
              float wg = w * gm[e];
              // the fp32 product must exist as a value of its own before it is rounded to fp16: left to itself the compiler turns
              // (half)(float(h) * g) into v_fma_mixlo_f16, whose result differed from the two roundings of the contract in about
              // 1 element of 10^4 on the MI355X (seen as ln_s, summed from that form, one fp16 ulp of one element away from the twin)
              asm volatile("" : "+v"(wg));
              out[e] = (half_t)wg;
              ps[q] = ps[q] + (float)out[e];
              const float wb = w * bt[e];
              pt[q] = pt[q] + wb;
            }
          }
          *reinterpret_cast<half8*>(dst + dr * kp + k) = out;
          if (copy_kind == VSD_LORA_COPY_RAW) *reinterpret_cast<half8*>(copy + (int64_t)row[q] * K + k) = wf;
          if (copy_kind == VSD_LORA_COPY_FRAG) *reinterpret_cast<half8*>(copy + lora_frag_off(dr, k, K)) = out;
        }
      }
    }
    if (gamma) {
#pragma unroll
      for (int q = 0; q < RPW; ++q) {
        float s = ps[q], t = pt[q];
#pragma unroll
        for (int h = LORA_LANES / 2; h >= 1; h >>= 1) {  // lanes below h hold the tree's p_l = p_l + p_{l+h}
          const float s2 = __shfl_xor(s, h, LORA_LANES), t2 = __shfl_xor(t, h, LORA_LANES);
          s = s + s2;
          t = t + t2;
        }
        if (lane == 0 && rbase + q < rows) {
          const int64_t dr = row0 + lora_map_row(map, rows, row[q]);
          g->ln_s[dr] = s;
          g->ln_t[dr] = g->bias ? t + g->bias[row[q]] : t;
        }
      }
    }
  }
}

// a table is read back ONCE per context, checked and remembered by address
int lora_table(vsd_ctx* ctx, const vsd_lora_seg* segs_dev, int nseg) {
  if (!segs_dev || ((uintptr_t)segs_dev & 15)) return vsd_fail(ctx, VSD_ERR_ARG, "lora_fuse: the segment table must be a 16-byte aligned device pointer");
  if (nseg < 1 || nseg > 65535) return vsd_fail(ctx, VSD_ERR_ARG, "lora_fuse: %d segments (1..65535)", nseg);
  auto it = ctx->lora_tables.find(segs_dev);
  if (it != ctx->lora_tables.end() && it->second == nseg) return VSD_OK;
  std::vector<vsd_lora_seg> host((size_t)nseg);
  VSD_HIP(ctx, hipMemcpy(host.data(), segs_dev, sizeof(vsd_lora_seg) * (size_t)nseg, hipMemcpyDeviceToHost));
  for (int i = 0; i < nseg; ++i)
    if (const char* why = lora_check_segment(host[i])) return vsd_fail(ctx, VSD_ERR_ARG, "lora_fuse: segment %d: %s", i, why);
  ctx->lora_tables[segs_dev] = nseg;
  return VSD_OK;
}

}  // namespace

extern "C" int vsd_lora_seg_size(void) { return (int)sizeof(vsd_lora_seg); }

extern "C" int vsd_lora_fuse_table(vsd_ctx* ctx, const vsd_lora_seg* segs_dev, int nseg) {
  if (!ctx) return VSD_ERR_ARG;
  if (nseg == 0) {  // forget this table (before its memory is freed or rewritten)
    ctx->lora_tables.erase(segs_dev);
    return VSD_OK;
  }
  return lora_table(ctx, segs_dev, nseg);
}

extern "C" int vsd_lora_fuse(vsd_ctx* ctx, const vsd_lora_seg* segs_dev, int nseg, const float* scales, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (const char* why = lora_check_scales(scales)) return vsd_fail(ctx, VSD_ERR_ARG, "lora_fuse: %s", why);
  if (int rc = lora_table(ctx, segs_dev, nseg)) return rc;
  LoraScales sc;
  for (int i = 0; i < VSD_LORA_MAX; ++i) sc.s[i] = scales[i];
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(LORA_BLOCKS_X, nseg), block(LORA_THREADS);
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(lora_fuse_kernel, grid, block, 0, s, segs_dev, sc);
  return ls.finish();
}

extern "C" int vsd_lora_fuse_host(const vsd_lora_seg* segs, int nseg, const float* scales) {
  const char* why;
  int bad;
  return lora_fuse_host(segs, nseg, scales, &why, &bad);
}
