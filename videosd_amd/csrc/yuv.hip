// Planar YUV 4:2:0 ("I420", what a decoded WebRTC frame is and what its encoder takes) <-> packed u8 RGB on the device and, with the
// same arithmetic, on the host (include/vsd.h vsd_i420_to_rgb* / vsd_rgb_to_i420*).  Replaces the two libswscale conversions of the
// reference's frame loop (server.py:108 `frame.to_image()`, server.py:117 `VideoFrame.from_image`).
//
// The colour contract is the project's own, stated in include/vsd.h: the published 8-bit integer form of BT.601 studio range, 32-bit
// integers, arithmetic shifts, one chroma sample per 2 x 2 luma block without interpolation.  Host loops and kernels call the SAME
// three inline functions below, and the tests hold both to a numpy statement of the formulas byte for byte.  How far libswscale's
// tables are from this contract is not measured anywhere in this tree.
// Form: integer elementwise code, no LDS, no atomics; a thread owns a strip of 4 pixels x 2 rows that shares its chroma row, and every
// output byte is written once with a plain vector store.  <true>: a dword of Y in and three dwords of RGB out per row (on the way
// back three dwords in, a dword of Y per row and a U and a V byte pair out); <false>: the same strip byte by byte, for pointers,
// strides and widths that are not multiples of 4 -- as resample_v_kernel<1> is to <4>.
#include <stdarg.h>  // (common.h's vsd_fail uses va_start and leaves the include to its users, as resample.hip and plan.hip do)

#include "common.h"

namespace {

__host__ __device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one pixel, I420 -> RGB; returns R | G << 8 | B << 16
__host__ __device__ __forceinline__ unsigned yuv_to_rgb(int y, int u, int v) {
  const int c = 298 * (y - 16) + 128, d = u - 128, e = v - 128;
  const int r = clamp255((c + 409 * e) >> 8);
  const int g = clamp255((c - 100 * d - 208 * e) >> 8);
  const int b = clamp255((c + 516 * d) >> 8);
  return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

__host__ __device__ __forceinline__ int rgb_to_y(int r, int g, int b) { return ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16; }
// (r, g, b: the rounded means of a 2 x 2 block)
__host__ __device__ __forceinline__ int rgb_to_u(int r, int g, int b) { return ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128; }
__host__ __device__ __forceinline__ int rgb_to_v(int r, int g, int b) { return ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128; }

struct ToRgbParams {
  const unsigned char *y, *u, *v;
  unsigned char* dst;
  long long y_stride, uv_stride, dst_stride;
  int px, py, h, w;  // parities of the rectangle's first luma sample
};

// Thread (tx, ty): columns 4 tx .. 4 tx + 3 of the rows whose chroma row is ty (two rows; one at an odd top edge or an odd bottom).
template <bool VEC>
__global__ void __launch_bounds__(256) i420_to_rgb_kernel(const ToRgbParams p) {
  const int j = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int cy = blockIdx.y * 4 + threadIdx.y;
  if (j >= p.w) return;
  const int r0 = 2 * cy - p.py;
  if (r0 >= p.h) return;
  // the strip's chroma samples: columns c0 .. c0 + 2 (the third only at an odd left edge), each read only if a pixel of the strip uses it
  const int n = p.w - j < 4 ? p.w - j : 4;
  const int c0 = (p.px + j) >> 1, nc = ((p.px + j + n - 1) >> 1) - c0 + 1;
  const unsigned char* us = p.u + (size_t)cy * p.uv_stride + c0;
  const unsigned char* vs = p.v + (size_t)cy * p.uv_stride + c0;
  int cu[3], cv[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    cu[k] = k < nc ? us[k] : 128;
    cv[k] = k < nc ? vs[k] : 128;
  }
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int r = r0 + rr;
    if (r < 0 || r >= p.h) continue;
    const unsigned char* ys = p.y + (size_t)r * p.y_stride + j;
    unsigned char* d = p.dst + (size_t)r * p.dst_stride + (size_t)j * 3;
    if (VEC && n == 4) {
      const unsigned yy = *reinterpret_cast<const unsigned*>(ys);
      unsigned px[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = (p.px + k) >> 1;  // (j is a multiple of 4: the strip's chroma index depends on k and the parity alone)
        px[k] = yuv_to_rgb((int)((yy >> (8 * k)) & 255u), c == 0 ? cu[0] : (c == 1 ? cu[1] : cu[2]), c == 0 ? cv[0] : (c == 1 ? cv[1] : cv[2]));
      }
      unsigned* d4 = reinterpret_cast<unsigned*>(d);
      d4[0] = px[0] | (px[1] << 24);
      d4[1] = (px[1] >> 8) | (px[2] << 16);
      d4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
      for (int k = 0; k < n; ++k) {
        const int c = (p.px + k) >> 1;
        const unsigned v = yuv_to_rgb((int)ys[k], c == 0 ? cu[0] : (c == 1 ? cu[1] : cu[2]), c == 0 ? cv[0] : (c == 1 ? cv[1] : cv[2]));
        d[3 * k] = (unsigned char)(v & 255u);
        d[3 * k + 1] = (unsigned char)((v >> 8) & 255u);
        d[3 * k + 2] = (unsigned char)(v >> 16);
      }
    }
  }
}

struct ToI420Params {
  const unsigned char* rgb;  // packed [h][w][3]
  unsigned char *y, *u, *v;
  long long y_stride, uv_stride;
  int h, w;  // both even
};

// Thread (tx, ty): columns 4 tx .. 4 tx + 3 (two at the right edge of a width that is 2 mod 4) of rows 2 ty and 2 ty + 1: two 2 x 2 blocks.
template <bool VEC>
__global__ void __launch_bounds__(256) rgb_to_i420_kernel(const ToI420Params p) {
  const int j = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int cy = blockIdx.y * 4 + threadIdx.y;
  const int r0 = 2 * cy;
  if (j >= p.w || r0 >= p.h) return;
  const int n = p.w - j < 4 ? p.w - j : 4;  // 4 or 2
  int sr[2] = {0, 0}, sg[2] = {0, 0}, sb[2] = {0, 0};
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const unsigned char* s = p.rgb + ((size_t)(r0 + rr) * p.w + j) * 3;
    unsigned char* yd = p.y + (size_t)(r0 + rr) * p.y_stride + j;
    if (VEC && n == 4) {
      const unsigned* s4 = reinterpret_cast<const unsigned*>(s);
      const unsigned a = s4[0], b = s4[1], c = s4[2];
      const int r[4] = {(int)(a & 255u), (int)(a >> 24), (int)((b >> 16) & 255u), (int)((c >> 8) & 255u)};
      const int g[4] = {(int)((a >> 8) & 255u), (int)(b & 255u), (int)(b >> 24), (int)((c >> 16) & 255u)};
      const int bl[4] = {(int)((a >> 16) & 255u), (int)((b >> 8) & 255u), (int)(c & 255u), (int)(c >> 24)};
      unsigned yy = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        yy |= (unsigned)rgb_to_y(r[k], g[k], bl[k]) << (8 * k);
        sr[k >> 1] += r[k];
        sg[k >> 1] += g[k];
        sb[k >> 1] += bl[k];
      }
      *reinterpret_cast<unsigned*>(yd) = yy;
    } else {
      for (int k = 0; k < n; ++k) {
        const int r = s[3 * k], g = s[3 * k + 1], b = s[3 * k + 2];
        yd[k] = (unsigned char)rgb_to_y(r, g, b);
        sr[k >> 1] += r;
        sg[k >> 1] += g;
        sb[k >> 1] += b;
      }
    }
  }
  unsigned char* ud = p.u + (size_t)cy * p.uv_stride + (j >> 1);
  unsigned char* vd = p.v + (size_t)cy * p.uv_stride + (j >> 1);
  const int u0 = rgb_to_u((sr[0] + 2) >> 2, (sg[0] + 2) >> 2, (sb[0] + 2) >> 2), v0 = rgb_to_v((sr[0] + 2) >> 2, (sg[0] + 2) >> 2, (sb[0] + 2) >> 2);
  if (n == 4) {
    const int u1 = rgb_to_u((sr[1] + 2) >> 2, (sg[1] + 2) >> 2, (sb[1] + 2) >> 2), v1 = rgb_to_v((sr[1] + 2) >> 2, (sg[1] + 2) >> 2, (sb[1] + 2) >> 2);
    if (VEC) {  // (the chroma planes and their stride are even in this form: a byte pair)
      *reinterpret_cast<unsigned short*>(ud) = (unsigned short)(u0 | (u1 << 8));
      *reinterpret_cast<unsigned short*>(vd) = (unsigned short)(v0 | (v1 << 8));
    } else {
      ud[0] = (unsigned char)u0;
      ud[1] = (unsigned char)u1;
      vd[0] = (unsigned char)v0;
      vd[1] = (unsigned char)v1;
    }
  } else {
    ud[0] = (unsigned char)u0;
    vd[0] = (unsigned char)v0;
  }
}

#define VSD_STR2(x) #x
#define VSD_STR(x) VSD_STR2(x)
const char* const kSides = "every side must be 1.." VSD_STR(VSD_RESAMPLE_MAX_SIDE);

inline bool side_ok(int v) { return v >= 1 && v <= VSD_RESAMPLE_MAX_SIDE; }
inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// bytes [p, p + (rows - 1) * stride + row) of a plane against those of another; rows >= 1 and stride >= row > 0 (the callers have
// checked sides and strides before they ask)
inline bool overlap(const void* a, long long a_stride, int a_rows, long long a_row, const void* b, long long b_stride, int b_rows, long long b_row) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)((a_rows - 1) * a_stride + a_row);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)((b_rows - 1) * b_stride + b_row);
  return a0 < b1 && b0 < a1;
}

// the checks the host loops and the launches share; a reason for every refusal
const char* to_rgb_refusal(const void* y, long long y_stride, const void* u, const void* v, long long uv_stride, int ox, int oy, int h, int w,
                           const void* dst, long long dst_row_bytes) {
  if (!y || !u || !v || !dst) return "null plane or destination";
  if (!side_ok(h) || !side_ok(w)) return kSides;
  if (ox < 0 || oy < 0) return "negative offset of the rectangle (ox, oy)";
  const int cw = ((ox & 1) + w + 1) >> 1, ch = ((oy & 1) + h + 1) >> 1;
  if (y_stride < w) return "y_stride shorter than a row of the rectangle";
  if (uv_stride < cw) return "uv_stride shorter than a chroma row of the rectangle";
  if (dst_row_bytes < (long long)3 * w) return "dst_row_bytes shorter than 3 * w";
  if (overlap(y, y_stride, h, w, dst, dst_row_bytes, h, 3LL * w) || overlap(u, uv_stride, ch, cw, dst, dst_row_bytes, h, 3LL * w) ||
      overlap(v, uv_stride, ch, cw, dst, dst_row_bytes, h, 3LL * w))
    return "a source plane overlaps the destination";
  return nullptr;
}

const char* to_i420_refusal(const void* rgb, int h, int w, const void* y, const void* u, const void* v, long long y_stride, long long uv_stride) {
  if (!rgb || !y || !u || !v) return "null source or plane";
  if (!side_ok(h) || !side_ok(w)) return kSides;
  if ((h | w) & 1) return "odd width or height: 4:2:0 output needs even sides";
  if (y_stride < w) return "y_stride shorter than a row";
  if (uv_stride < w / 2) return "uv_stride shorter than a chroma row";
  if (overlap(rgb, 3LL * w, h, 3LL * w, y, y_stride, h, w) || overlap(rgb, 3LL * w, h, 3LL * w, u, uv_stride, h / 2, w / 2) ||
      overlap(rgb, 3LL * w, h, 3LL * w, v, uv_stride, h / 2, w / 2))
    return "the source overlaps a destination plane";
  if (overlap(y, y_stride, h, w, u, uv_stride, h / 2, w / 2) || overlap(y, y_stride, h, w, v, uv_stride, h / 2, w / 2) ||
      overlap(u, uv_stride, h / 2, w / 2, v, uv_stride, h / 2, w / 2))
    return "destination planes overlap each other";
  return nullptr;
}

}  // namespace

extern "C" int vsd_i420_to_rgb_host(const void* y, int64_t y_stride, const void* u, const void* v, int64_t uv_stride, int ox, int oy, int h, int w,
                                    void* dst_rgb, int64_t dst_row_bytes) {
  if (to_rgb_refusal(y, y_stride, u, v, uv_stride, ox, oy, h, w, dst_rgb, dst_row_bytes)) return VSD_ERR_ARG;
  const int px = ox & 1, py = oy & 1;
  for (int i = 0; i < h; ++i) {
    const unsigned char* ys = (const unsigned char*)y + (size_t)i * y_stride;
    const unsigned char* us = (const unsigned char*)u + (size_t)((py + i) >> 1) * uv_stride;
    const unsigned char* vs = (const unsigned char*)v + (size_t)((py + i) >> 1) * uv_stride;
    unsigned char* d = (unsigned char*)dst_rgb + (size_t)i * dst_row_bytes;
    for (int j = 0; j < w; ++j) {
      const unsigned p = yuv_to_rgb(ys[j], us[(px + j) >> 1], vs[(px + j) >> 1]);
      d[3 * j] = (unsigned char)(p & 255u);
      d[3 * j + 1] = (unsigned char)((p >> 8) & 255u);
      d[3 * j + 2] = (unsigned char)(p >> 16);
    }
  }
  return VSD_OK;
}

extern "C" int vsd_rgb_to_i420_host(const void* rgb_u8, int h, int w, void* dst_y, void* dst_u, void* dst_v, int64_t y_stride, int64_t uv_stride) {
  if (to_i420_refusal(rgb_u8, h, w, dst_y, dst_u, dst_v, y_stride, uv_stride)) return VSD_ERR_ARG;
  const unsigned char* s = (const unsigned char*)rgb_u8;
  for (int i = 0; i < h; ++i) {
    unsigned char* yd = (unsigned char*)dst_y + (size_t)i * y_stride;
    for (int j = 0; j < w; ++j) {
      const unsigned char* q = s + ((size_t)i * w + j) * 3;
      yd[j] = (unsigned char)rgb_to_y(q[0], q[1], q[2]);
    }
  }
  for (int i = 0; i < h / 2; ++i) {
    unsigned char* ud = (unsigned char*)dst_u + (size_t)i * uv_stride;
    unsigned char* vd = (unsigned char*)dst_v + (size_t)i * uv_stride;
    const unsigned char *a = s + (size_t)(2 * i) * w * 3, *b = a + (size_t)w * 3;
    for (int j = 0; j < w / 2; ++j) {
      int m[3];
      for (int c = 0; c < 3; ++c) m[c] = (a[6 * j + c] + a[6 * j + 3 + c] + b[6 * j + c] + b[6 * j + 3 + c] + 2) >> 2;
      ud[j] = (unsigned char)rgb_to_u(m[0], m[1], m[2]);
      vd[j] = (unsigned char)rgb_to_v(m[0], m[1], m[2]);
    }
  }
  return VSD_OK;
}

extern "C" int vsd_i420_to_rgb(vsd_ctx* ctx, const void* y, int64_t y_stride, const void* u, const void* v, int64_t uv_stride, int ox, int oy, int h, int w,
                               void* dst_rgb, int64_t dst_row_bytes, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (const char* why = to_rgb_refusal(y, y_stride, u, v, uv_stride, ox, oy, h, w, dst_rgb, dst_row_bytes))
    return vsd_fail(ctx, VSD_ERR_ARG, "i420_to_rgb: %d x %d at (%d, %d), strides %lld / %lld -> rows of %lld bytes: %s", w, h, ox, oy, (long long)y_stride,
                    (long long)uv_stride, (long long)dst_row_bytes, why);
  ToRgbParams p;
  p.y = (const unsigned char*)y;
  p.u = (const unsigned char*)u;
  p.v = (const unsigned char*)v;
  p.dst = (unsigned char*)dst_rgb;
  p.y_stride = y_stride;
  p.uv_stride = uv_stride;
  p.dst_stride = dst_row_bytes;
  p.px = ox & 1;
  p.py = oy & 1;
  p.h = h;
  p.w = w;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope scope(ctx, s, VSD_FAM_ELEMENTWISE, 0);
  const dim3 grid(cdiv(cdiv(w, 4), 64), cdiv((p.py + h + 1) >> 1, 4)), block(64, 4);
  if (aligned(y, 4) && aligned(dst_rgb, 4) && y_stride % 4 == 0 && dst_row_bytes % 4 == 0)
    hipLaunchKernelGGL(i420_to_rgb_kernel<true>, grid, block, 0, s, p);
  else
    hipLaunchKernelGGL(i420_to_rgb_kernel<false>, grid, block, 0, s, p);
  return scope.finish();
}

extern "C" int vsd_rgb_to_i420(vsd_ctx* ctx, const void* rgb_u8, int h, int w, void* dst_y, void* dst_u, void* dst_v, int64_t y_stride, int64_t uv_stride,
                               void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (const char* why = to_i420_refusal(rgb_u8, h, w, dst_y, dst_u, dst_v, y_stride, uv_stride))
    return vsd_fail(ctx, VSD_ERR_ARG, "rgb_to_i420: %d x %d -> strides %lld / %lld: %s", w, h, (long long)y_stride, (long long)uv_stride, why);
  ToI420Params p;
  p.rgb = (const unsigned char*)rgb_u8;
  p.y = (unsigned char*)dst_y;
  p.u = (unsigned char*)dst_u;
  p.v = (unsigned char*)dst_v;
  p.y_stride = y_stride;
  p.uv_stride = uv_stride;
  p.h = h;
  p.w = w;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope scope(ctx, s, VSD_FAM_ELEMENTWISE, 0);
  const dim3 grid(cdiv(cdiv(w, 4), 64), cdiv(h / 2, 4)), block(64, 4);
  // (rows of 3 * w bytes start on a dword when w is a multiple of 4)
  if (aligned(rgb_u8, 4) && w % 4 == 0 && aligned(dst_y, 4) && y_stride % 4 == 0 && aligned(dst_u, 2) && aligned(dst_v, 2) && uv_stride % 2 == 0)
    hipLaunchKernelGGL(rgb_to_i420_kernel<true>, grid, block, 0, s, p);
  else
    hipLaunchKernelGGL(rgb_to_i420_kernel<false>, grid, block, 0, s, p);
  return scope.finish();
}
