// Canny edges for the ControlNet on the device (include/vsd.h THE EDGE CONTRACT): gray value, 3 x 3 Sobel, L1 magnitude, non-maximum
// suppression, two thresholds, hysteresis over 8-connected components.  control_v11p_sd15_canny was trained on such maps; the default
// program keeps the reference's Sobel stand-in (csrc/elementwise.hip vsd_sobel_control) and this is the opt-in alternative.
//
// The arithmetic and the label steps live in canny_core.h, shared with the host twin and with scripts/canny_model.cpp; the kernels here
// are loops over those steps.  Four launches per call, always: the number does not depend on the content, nothing waits for the host or
// for another workgroup, nothing needs zeroing ahead (launch 1 writes every word of the workspace the later ones read).
// Form: integer elementwise code.  Launch 1 reads the frame byte by byte (three bytes per pixel, any alignment) into LDS; launches 2 and 3
// touch one int / byte per pixel; launch 4 writes one 16-byte row of the conditioning tensor per thread.
#include <stdarg.h>  // (common.h's vsd_fail uses va_start and leaves the include to its users)

#include "canny_core.h"
#include "common.h"

static_assert(CANNY_MAX_SIDE == VSD_RESAMPLE_MAX_SIDE, "one limit for the sides of a frame");

namespace {

constexpr int CANNY_THREADS = 256;

// every loop below runs a fixed number of trips (a range divided among the threads); the barriers are reached by all threads
__global__ void __launch_bounds__(CANNY_THREADS) canny_tile_kernel(const unsigned char* __restrict__ rgb, int h, int w, int low, int high,
                                                                   int* __restrict__ parent, unsigned char* __restrict__ strong,
                                                                   unsigned char* __restrict__ flag) {
  __shared__ CannyTile t;
  const int x0 = blockIdx.x * CANNY_TW, y0 = blockIdx.y * CANNY_TH, tid = threadIdx.x;
  for (int q = tid; q < CANNY_GRAY_N; q += CANNY_THREADS) canny_tile_gray(t, rgb, h, w, x0, y0, q);
  __syncthreads();
  for (int q = tid; q < CANNY_MAG_N; q += CANNY_THREADS) canny_tile_mag(t, h, w, x0, y0, q);
  __syncthreads();
  for (int q = tid; q < CANNY_TILE_N; q += CANNY_THREADS) canny_tile_class(t, h, w, x0, y0, low, high, q);
  __syncthreads();
  for (int q = tid; q < CANNY_TILE_N; q += CANNY_THREADS) canny_tile_unite(t, q);  // (canny_unite / canny_find: bounded by their own arguments)
  __syncthreads();
  for (int q = tid; q < CANNY_TILE_N; q += CANNY_THREADS) canny_tile_write(t, h, w, x0, y0, q, parent, strong, flag);
}

// `parent` is not __restrict__ / const here: other workgroups lower its words during this launch (canny_core.h CANNY_LOAD)
__global__ void __launch_bounds__(CANNY_THREADS) canny_border_kernel(int* parent, int h, int w) {
  const int i = blockIdx.x * CANNY_THREADS + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  if (canny_on_tile_border(x, y)) canny_border_unite(parent, h, w, x, y);
}

__global__ void __launch_bounds__(CANNY_THREADS) canny_mark_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ strong,
                                                                   unsigned char* __restrict__ flag, int n) {
  const int i = blockIdx.x * CANNY_THREADS + threadIdx.x;
  if (i < n) canny_mark(parent, strong, flag, i);
}

__global__ void __launch_bounds__(CANNY_THREADS) canny_write_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ flag, int n,
                                                                    unsigned char* __restrict__ edge, half_t* __restrict__ ctrl) {
  const int i = blockIdx.x * CANNY_THREADS + threadIdx.x;
  if (i >= n) return;
  const bool e = canny_is_edge(parent, flag, i);
  edge[i] = e ? 255 : 0;
  const half_t v = e ? (half_t)1.0f : (half_t)0.0f;
  *reinterpret_cast<half8*>(ctrl + (size_t)i * 8) = (half8){v, v, v, 0, 0, 0, 0, 0};
}

}  // namespace

extern "C" int64_t vsd_canny_workspace_bytes(int h, int w) { return canny_workspace_bytes(h, w); }

extern "C" int vsd_canny_host(const void* rgb_u8, int h, int w, int low, int high, void* edge_u8) {
  return canny_host((const unsigned char*)rgb_u8, h, w, low, high, (unsigned char*)edge_u8) ? VSD_OK : VSD_ERR_ARG;
}

extern "C" int vsd_canny_control(vsd_ctx* ctx, const void* rgb_u8, int h, int w, int low, int high, void* edge_u8, void* control_out, void* workspace,
                                 void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!rgb_u8 || !edge_u8 || !control_out || !workspace) return vsd_fail(ctx, VSD_ERR_ARG, "canny_control: null pointer");
  if (!canny_args_ok(h, w, low, high))
    return vsd_fail(ctx, VSD_ERR_ARG, "canny_control: %d x %d, thresholds (%d, %d): sides must be 1..%d and 0 <= low <= high <= %d", w, h, low, high,
                    CANNY_MAX_SIDE, CANNY_MAX_MAG);
  if (((uintptr_t)workspace & 3) || ((uintptr_t)control_out & 15))
    return vsd_fail(ctx, VSD_ERR_ARG, "canny_control: workspace must be 4-byte aligned and control_out 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int n = h * w;
  int* parent = (int*)workspace;
  unsigned char* strong = (unsigned char*)workspace + (size_t)n * 4;
  unsigned char* flag = strong + n;
  const dim3 block(CANNY_THREADS), tiles(cdiv(w, CANNY_TW), cdiv(h, CANNY_TH)), pixels(cdiv(n, CANNY_THREADS));
  {
    LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
    hipLaunchKernelGGL(canny_tile_kernel, tiles, block, 0, s, (const unsigned char*)rgb_u8, h, w, low, high, parent, strong, flag);
    if (int rc = ls.finish()) return rc;
  }
  {
    LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
    hipLaunchKernelGGL(canny_border_kernel, pixels, block, 0, s, parent, h, w);
    if (int rc = ls.finish()) return rc;
  }
  {
    LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
    hipLaunchKernelGGL(canny_mark_kernel, pixels, block, 0, s, (const int*)parent, (const unsigned char*)strong, flag, n);
    if (int rc = ls.finish()) return rc;
  }
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(canny_write_kernel, pixels, block, 0, s, (const int*)parent, (const unsigned char*)flag, n, (unsigned char*)edge_u8, (half_t*)control_out);
  return ls.finish();
}
