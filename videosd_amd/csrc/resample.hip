// Centre crop + LANCZOS resize of a packed u8 RGB frame on the device, bit for bit Pillow's `img.crop(box).resize(size, LANCZOS)`
// (include/vsd.h vsd_resample_*).  Replaces the PIL crop + resize in front of every frame of the reference (videopipeline.py:92-107).
//
// Pillow's 8-bit resample is integer arithmetic on tables of 22-bit fixed-point weights:
//   * the tables are built HERE ON THE HOST, in double, with the C library's sin -- the same libm Pillow calls, so the same last bit
//     (a table computed on the GPU, or with another sin, differs in the last bit of a few weights and then in a few bytes);
//   * a pass along one axis is  clamp((2^21 + sum pixel * k) >> 22, 0, 255)  in 32-bit integers;
//   * horizontal pass first into an 8-BIT intermediate, vertical pass second: the intermediate rounding is part of the result, the
//     two passes cannot be merged into one 2-D filter.  A pass whose input length equals its output length is skipped.
// Form: one launch per pass, the intermediate ([box height][dst width] pixels, ~1 MB for 1280 x 720 -> 512 x 512: L2-resident) in a
// caller-owned workspace.  No LDS, no atomics: every output byte is written once by one thread with a plain vector store.
// (Both passes as ONE launch with the intermediate in LDS -- a workgroup per 16 x 64 output pixels -- gives the same bytes and measured
// slower, 15.3 against 12.1 us per 1280 x 720 frame: the blocks repeat the horizontal pass of the rows they share.  docs/NOTEBOOK.md.)
#include <math.h>
#include <stdarg.h>

#include "common.h"

#define VSD_RESAMPLE_PRECISION_BITS 22

// The host arithmetic of this file restates Python / Pillow expression by expression: no fused multiply-adds, whatever the host target
// (the kernels are integer code).
#pragma clang fp contract(off)

namespace {

inline double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

inline double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

inline bool side_ok(int v) { return v >= 1 && v <= VSD_RESAMPLE_MAX_SIDE; }

// ksize of the (in -> out) table; 0 for sizes outside the limits
int table_ksize(int in, int out) {
  if (!side_ok(in) || !side_ok(out)) return 0;
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 3.0 * fs;
  return (int)ceil(support) * 2 + 1;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the whole input range [0, in)
int table_fill(int in, int out, int32_t* xmin_out, int32_t* count_out, int32_t* coeffs) {
  const int ksize = table_ksize(in, out);
  if (ksize <= 0) return 0;
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 3.0 * fs;
  std::vector<double> w((size_t)ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      w[x] = lanczos_filter((x + xmin - center + 0.5) / fs);
      ww += w[x];
    }
    int32_t* k = coeffs + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      double v = 0.0;
      if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
      k[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << VSD_RESAMPLE_PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << VSD_RESAMPLE_PRECISION_BITS));
    }
    xmin_out[xx] = xmin;
    count_out[xx] = xmax;
  }
  return ksize;
}

struct ResampleParams {
  const unsigned char* src;  // first byte of the first line the pass reads
  unsigned char* dst;
  long long src_stride, dst_stride;  // bytes per row
  const int32_t* xmin;               // the axis' table: [out] first tap, [out] tap count, [out][ksize] weights
  const int32_t* count;
  const int32_t* k;
  int ksize, in, out, lines;  // taps per output, input / output length along the axis, pixels (h pass) or bytes (v pass) across it
};

__device__ __forceinline__ unsigned char clip8(int acc) {
  const int v = acc >> VSD_RESAMPLE_PRECISION_BITS;  // (arithmetic shift, as Pillow's)
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Horizontal pass: one thread per output pixel (three channels share the weights).  block (64, 4): 64 consecutive output columns of 4 rows.
__global__ void __launch_bounds__(256) resample_h_kernel(const ResampleParams p) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x >= p.out || y >= p.lines) return;
  // (the table is the caller's memory: whatever it holds, no tap leaves the line)
  int x0 = p.xmin[x], n = p.count[x];
  x0 = x0 < 0 ? 0 : (x0 > p.in ? p.in : x0);
  n = n < 0 ? 0 : n;
  n = n > p.ksize ? p.ksize : n;
  n = n > p.in - x0 ? p.in - x0 : n;
  const int32_t* k = p.k + (size_t)x * p.ksize;
  const unsigned char* s = p.src + (size_t)y * p.src_stride + (size_t)x0 * 3;
  int a0 = 1 << (VSD_RESAMPLE_PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < n; ++t) {
    const int kk = k[t];
    a0 += (int)s[3 * t] * kk;
    a1 += (int)s[3 * t + 1] * kk;
    a2 += (int)s[3 * t + 2] * kk;
  }
  unsigned char* d = p.dst + (size_t)y * p.dst_stride + (size_t)x * 3;
  d[0] = clip8(a0);
  d[1] = clip8(a1);
  d[2] = clip8(a2);
}

// Vertical pass: a workgroup owns 256 * V consecutive bytes of ONE output row, so the weights are uniform over the workgroup (scalar
// loads) and the taps are coalesced row reads.  V = 4: a dword per tap and thread (pointers, strides and width multiples of 4).
template <int V>
__global__ void __launch_bounds__(256) resample_v_kernel(const ResampleParams p) {
  const int b = (blockIdx.x * 256 + threadIdx.x) * V;
  const int y = blockIdx.y;
  if (b >= p.lines || y >= p.out) return;
  int y0 = p.xmin[y], n = p.count[y];
  y0 = y0 < 0 ? 0 : (y0 > p.in ? p.in : y0);
  n = n < 0 ? 0 : n;
  n = n > p.ksize ? p.ksize : n;
  n = n > p.in - y0 ? p.in - y0 : n;
  const int32_t* k = p.k + (size_t)y * p.ksize;
  const unsigned char* s = p.src + (size_t)y0 * p.src_stride + b;
  unsigned char* d = p.dst + (size_t)y * p.dst_stride + b;
  if constexpr (V == 4) {
    int a0 = 1 << (VSD_RESAMPLE_PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int t = 0; t < n; ++t) {
      const int kk = k[t];
      const unsigned v = *reinterpret_cast<const unsigned*>(s + (size_t)t * p.src_stride);
      a0 += (int)(v & 255u) * kk;
      a1 += (int)((v >> 8) & 255u) * kk;
      a2 += (int)((v >> 16) & 255u) * kk;
      a3 += (int)(v >> 24) * kk;
    }
    *reinterpret_cast<unsigned*>(d) = (unsigned)clip8(a0) | ((unsigned)clip8(a1) << 8) | ((unsigned)clip8(a2) << 16) | ((unsigned)clip8(a3) << 24);
  } else {
    int a0 = 1 << (VSD_RESAMPLE_PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) a0 += (int)s[(size_t)t * p.src_stride] * k[t];
    d[0] = clip8(a0);
  }
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace

// Rule of videopipeline.py:92-107 + PIL's Image.crop: the float box in Python's expression order, then int(round(v)) per edge, and
// Python's round is half to even (rint in the default rounding mode, not round).
extern "C" int vsd_center_crop_box(int src_w, int src_h, int dst_w, int dst_h, int* box) {
  if (!box || src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1) return VSD_ERR_ARG;
  const double iw = src_w, ih = src_h, w = dst_w, h = dst_h;
  double b[4];
  if (iw / ih > w / h) {
    const double new_width = ih * (w / h);
    b[0] = (iw - new_width) / 2;
    b[1] = 0;
    b[2] = (iw + new_width) / 2;
    b[3] = ih;
  } else {
    const double new_height = iw * (h / w);
    b[0] = 0;
    b[1] = (ih - new_height) / 2;
    b[2] = iw;
    b[3] = (ih + new_height) / 2;
  }
  for (int i = 0; i < 4; ++i) box[i] = (int)rint(b[i]);
  return VSD_OK;
}
extern "C" int64_t vsd_resample_table_bytes(int in, int out) {
  const int ksize = table_ksize(in, out);
  return ksize <= 0 ? 0 : (int64_t)sizeof(int32_t) * out * (2 + ksize);
}

extern "C" int vsd_resample_table_host(int in, int out, int32_t* xmin, int32_t* count, int32_t* coeffs) {
  if (!xmin || !count || !coeffs) return VSD_ERR_ARG;
  const int ksize = table_fill(in, out, xmin, count, coeffs);
  return ksize > 0 ? ksize : VSD_ERR_ARG;
}

extern "C" int vsd_resample_table_upload(vsd_ctx* ctx, int in, int out, void* table_dev, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  const int64_t bytes = vsd_resample_table_bytes(in, out);
  if (!table_dev || bytes <= 0)
    return vsd_fail(ctx, VSD_ERR_ARG, "resample_table_upload: %d -> %d: both lengths must be 1..%d and the table pointer non-null", in, out, VSD_RESAMPLE_MAX_SIDE);
  std::vector<int32_t> host((size_t)bytes / sizeof(int32_t));
  table_fill(in, out, host.data(), host.data() + out, host.data() + 2 * (size_t)out);
  // (the host buffer is a temporary: the copy has left it when this returns.  A table is built when a camera changes resolution, not per frame.)
  VSD_HIP(ctx, hipMemcpyAsync(table_dev, host.data(), (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  VSD_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
  return VSD_OK;
}

extern "C" int64_t vsd_resample_workspace_bytes(int box_h, int dst_w) {
  if (!side_ok(box_h) || !side_ok(dst_w)) return 0;
  return (int64_t)box_h * dst_w * 3;
}

extern "C" int vsd_resample_rgb(vsd_ctx* ctx, const void* src_u8, int src_h, int src_w, int64_t src_row_bytes, const int* box, void* dst_u8,
                                int dst_h, int dst_w, const void* table_x, const void* table_y, void* workspace, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!src_u8 || !dst_u8 || !box) return vsd_fail(ctx, VSD_ERR_ARG, "resample_rgb: null source, destination or box");
  if (!side_ok(src_h) || !side_ok(src_w) || !side_ok(dst_h) || !side_ok(dst_w))
    return vsd_fail(ctx, VSD_ERR_ARG, "resample_rgb: %d x %d -> %d x %d: every side must be 1..%d", src_w, src_h, dst_w, dst_h, VSD_RESAMPLE_MAX_SIDE);
  if (src_row_bytes < (int64_t)3 * src_w) return vsd_fail(ctx, VSD_ERR_ARG, "resample_rgb: src_row_bytes %lld < 3 * %d", (long long)src_row_bytes, src_w);
  const int bx = box[0], by = box[1], bw = box[2] - box[0], bh = box[3] - box[1];
  if (bx < 0 || by < 0 || bw < 1 || bh < 1 || box[2] > src_w || box[3] > src_h)
    return vsd_fail(ctx, VSD_ERR_ARG, "resample_rgb: box (%d, %d, %d, %d) is empty or leaves the %d x %d source", box[0], box[1], box[2], box[3], src_w, src_h);
  const bool pass_x = bw != dst_w, pass_y = bh != dst_h;
  if ((pass_x && !table_x) || (pass_y && !table_y)) return vsd_fail(ctx, VSD_ERR_ARG, "resample_rgb: %d x %d -> %d x %d needs a table for each axis it resamples", bw, bh, dst_w, dst_h);
  if (pass_x && pass_y && !workspace) return vsd_fail(ctx, VSD_ERR_ARG, "resample_rgb: two passes need a workspace (vsd_resample_workspace_bytes)");
  hipStream_t s = (hipStream_t)stream;
  const unsigned char* src = (const unsigned char*)src_u8 + (size_t)by * src_row_bytes + (size_t)bx * 3;
  const long long dst_stride = (long long)dst_w * 3;
  if (!pass_x && !pass_y) {  // the box IS the target: Pillow copies
    VSD_HIP(ctx, hipMemcpy2DAsync(dst_u8, (size_t)dst_stride, src, (size_t)src_row_bytes, (size_t)dst_stride, (size_t)dst_h, hipMemcpyDeviceToDevice, s));
    return VSD_OK;
  }
  auto table = [](ResampleParams& p, const void* t, int in, int out) {
    p.xmin = (const int32_t*)t;
    p.count = p.xmin + out;
    p.k = p.xmin + 2 * (size_t)out;
    p.ksize = table_ksize(in, out);
    p.in = in;
    p.out = out;
  };
  LaunchScope scope(ctx, s, VSD_FAM_ELEMENTWISE, 0);
  const unsigned char* vsrc = src;
  long long vsrc_stride = src_row_bytes;
  if (pass_x) {
    ResampleParams p;
    table(p, table_x, bw, dst_w);
    p.src = src;
    p.src_stride = src_row_bytes;
    p.dst = pass_y ? (unsigned char*)workspace : (unsigned char*)dst_u8;
    p.dst_stride = dst_stride;
    p.lines = bh;
    hipLaunchKernelGGL(resample_h_kernel, dim3(cdiv(dst_w, 64), cdiv(bh, 4)), dim3(64, 4), 0, s, p);
    vsrc = p.dst;
    vsrc_stride = dst_stride;
  }
  if (pass_y) {
    ResampleParams p;
    table(p, table_y, bh, dst_h);
    p.src = vsrc;
    p.src_stride = vsrc_stride;
    p.dst = (unsigned char*)dst_u8;
    p.dst_stride = dst_stride;
    p.lines = dst_w * 3;
    if (aligned4(p.src) && aligned4(p.dst) && p.src_stride % 4 == 0 && p.dst_stride % 4 == 0)
      hipLaunchKernelGGL(resample_v_kernel<4>, dim3(cdiv(p.lines, 1024), dst_h), dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL(resample_v_kernel<1>, dim3(cdiv(p.lines, 256), dst_h), dim3(256), 0, s, p);
  }
  return scope.finish();
}
