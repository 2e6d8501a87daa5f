// A small Gaussian blur of packed u8 frames on the device (include/vsd.h THE BLUR CONTRACT): what calms the camera frame ahead of the
// edge op and feathers a keep mask ahead of the mask stages, inside the recorded program.
//
// The rounding expressions, the clamp, the tile's source span and the walk over a row live in blur_core.h, shared with the host twin and
// with scripts/blur_model.cpp; the kernel here is two loops over those.  ONE launch for all frames of the call: one workgroup per
// BLUR_TILE_H x BLUR_TILE_W-byte tile of one frame (blockIdx.z = frame).  Horizontal pass from global memory into an LDS image of u16
// (the tile's rows plus R halo rows above and below, rows clamped), one barrier, vertical pass from LDS to global memory: no
// intermediate goes to global memory, no workspace, no atomics.
// Form: integer code; per output byte 2R + 1 multiply-adds in either pass.  A row is C*w bytes, so neighbouring lanes read neighbouring
// bytes for C = 1 and C = 3 alike.  Horizontal: a lane takes four neighbouring bytes and cuts every tap's four source bytes out of a
// sliding window of two aligned 4-byte words (R*C/2 + 2 word loads instead of 4 (2R + 1) byte loads); bytes with a clamped tap, the
// ends of a row and groups whose words would reach outside the operand go one byte at a time.  Vertical: four u16 columns per lane as
// one 8-byte LDS read per tap (the 8 lanes of a row cover its 64 bytes, 64 lanes eight consecutive rows: no bank conflict), one word store where the destination is 4-byte
// aligned, its four bytes one by one elsewhere (the compiler may merge those into one unaligned store of exactly these four bytes);
// no store reaches past a row's end.  The LDS image is sized for R = 32 (8 KB, see blur_core.h); the
// loops run over the table's own R, clamped into 1..32, so no table can index outside the image.
// The taps are read once per wave: lane l holds word l of the table, and a tap is a v_readlane of it.
#include <stdarg.h>  // (common.h's vsd_fail uses va_start and leaves the include to its users)

#include "common.h"
#include "blur_core.h"

static_assert(BLUR_MAX_SIDE == VSD_RESAMPLE_MAX_SIDE && BLUR_MAX_RADIUS == VSD_BLUR_MAX_RADIUS && BLUR_ONE == VSD_BLUR_ONE, "one set of limits");

namespace {

constexpr int BL_THREADS = 256;
constexpr int BL_GROUPS = BLUR_TILE_W / BLUR_GROUP;  // groups of a tile row
static_assert(BLUR_TAPS <= 64, "one lane per word of the table");

struct LaneTaps {  // lane l of the wave holds word l of the table; tap k = word 1 + k
  int v;
  __device__ __forceinline__ int operator()(int k) const { return __builtin_amdgcn_readlane(v, 1 + k); }
};

struct GlobalWord {
  __device__ __forceinline__ uint32_t operator()(uintptr_t a) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>(a); }
};

// grid (blur_tiles_x, blur_tiles_y, frames)
__global__ void __launch_bounds__(BL_THREADS) gauss_blur_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int frames, int h,
                                                                int w, int C, const int* __restrict__ taps) {
  __shared__ __attribute__((aligned(16))) uint16_t image[BLUR_LDS_ROWS * BLUR_TILE_W];
  const int tid = threadIdx.x, lane = tid & 63;
  LaneTaps tap{taps[lane < BLUR_TAPS ? lane : BLUR_TAPS - 1]};
  const int R = blur_radius(__builtin_amdgcn_readlane(tap.v, 0));
  const BlurTile t = blur_tile(h, w, C, R, (int)blockIdx.x, (int)blockIdx.y);
  const int rb = C * w;
  const size_t frame = (size_t)h * rb;
  const unsigned char* sf = src + (size_t)blockIdx.z * frame;
  unsigned char* df = dst + (size_t)blockIdx.z * frame;
  const uintptr_t lo = (uintptr_t)src, hi = lo + (size_t)frames * frame;

  for (int s = tid; s < t.rows * BL_GROUPS; s += BL_THREADS) {
    const int r = s / BL_GROUPS, col = (s - r * BL_GROUPS) * BLUR_GROUP, b = t.c0 + col;
    if (b >= t.c1) continue;
    const unsigned char* row = sf + (size_t)blur_lds_src_row(t, R, r, h) * rb;
    uint16_t* o = image + r * BLUR_TILE_W + col;
    if (blur_group_words(t, b, (uintptr_t)row, lo, hi, R, C)) {
      uint32_t q[BLUR_GROUP];
      blur_h_group((uintptr_t)row, b, C, R, tap, GlobalWord(), q);
      *reinterpret_cast<uint2*>(o) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
    } else {
      for (int k = 0; k < BLUR_GROUP && b + k < t.c1; ++k) o[k] = (uint16_t)blur_h_byte(row, b + k, w, C, R, tap);
    }
  }
  __syncthreads();
  for (int s = tid; s < (t.y1 - t.y0) * BL_GROUPS; s += BL_THREADS) {
    const int yy = s / BL_GROUPS, col = (s - yy * BL_GROUPS) * BLUR_GROUP, b = t.c0 + col;
    if (b >= t.c1) continue;
    const uint16_t* c = image + yy * BLUR_TILE_W + col;  // LDS row yy = source row y - R
    unsigned char* d = df + (size_t)(t.y0 + yy) * rb + b;
    if (b + BLUR_GROUP <= t.c1) {
      uint32_t V[BLUR_GROUP] = {0, 0, 0, 0};
      for (int j = 0; j <= 2 * R; ++j) {
        const uint2 q = *reinterpret_cast<const uint2*>(c + j * BLUR_TILE_W);
        const uint32_t wt = (uint32_t)tap(j < R ? R - j : j - R);
        V[0] = blur_mac(V[0], wt, q.x & 0xffffu);
        V[1] = blur_mac(V[1], wt, q.x >> 16);
        V[2] = blur_mac(V[2], wt, q.y & 0xffffu);
        V[3] = blur_mac(V[3], wt, q.y >> 16);
      }
      const uint32_t word = blur_round_v(V[0]) | (blur_round_v(V[1]) << 8) | (blur_round_v(V[2]) << 16) | (blur_round_v(V[3]) << 24);
      if (((uintptr_t)d & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d) = word;
      } else {
#pragma unroll
        for (int k = 0; k < BLUR_GROUP; ++k) d[k] = (unsigned char)(word >> (8 * k));
      }
    } else {
      for (int k = 0; b + k < t.c1; ++k) d[k] = blur_v_byte(c + k, BLUR_TILE_W, R, tap);
    }
  }
}

}  // namespace

extern "C" int vsd_gauss_blur_host(const void* src_u8, void* dst_u8, int frames, int h, int w, int channels, const int32_t* taps) {
  return blur_host((const unsigned char*)src_u8, (unsigned char*)dst_u8, frames, h, w, channels, taps) ? VSD_OK : VSD_ERR_ARG;
}

extern "C" int vsd_gauss_blur(vsd_ctx* ctx, const void* src_u8, void* dst_u8, int frames, int h, int w, int channels, const void* taps_dev,
                              void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!src_u8 || !dst_u8 || !taps_dev || ((uintptr_t)taps_dev & 3)) return vsd_fail(ctx, VSD_ERR_ARG, "gauss_blur: null pointer, or taps_dev not 4-byte aligned");
  if (!blur_args_ok(frames, h, w, channels))
    return vsd_fail(ctx, VSD_ERR_ARG, "gauss_blur: %d frame(s) of %d x %d x %d: frames must be 1..%d, sides 1..%d, channels 1 or 3", frames, w, h, channels,
                    BLUR_MAX_FRAMES, BLUR_MAX_SIDE);
  const size_t bytes = (size_t)frames * h * w * channels;
  const uintptr_t s0 = (uintptr_t)src_u8, d0 = (uintptr_t)dst_u8;
  if (s0 < d0 + bytes && d0 < s0 + bytes) return vsd_fail(ctx, VSD_ERR_ARG, "gauss_blur: src and dst overlap");
  const int tx = blur_tiles_x(w, channels), ty = blur_tiles_y(h);
  if ((int64_t)tx * ty * frames > BLUR_MAX_TILES)
    return vsd_fail(ctx, VSD_ERR_ARG, "gauss_blur: %d frame(s) of %d x %d x %d are more than %d tiles of %d rows x %d bytes: split the call", frames, w, h,
                    channels, BLUR_MAX_TILES, BLUR_TILE_H, BLUR_TILE_W);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(gauss_blur_kernel, dim3(tx, ty, frames), dim3(BL_THREADS), 0, s, (const unsigned char*)src_u8, (unsigned char*)dst_u8, frames, h, w,
                     channels, (const int*)taps_dev);
  return ls.finish();
}
