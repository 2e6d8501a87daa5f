// The scheduler arithmetic and the seeded noise that can feed it (include/vsd.h: THE SCHEDULER ARITHMETIC, THE NOISE CONTRACT).
// One add_noise body and one lcm_step body serve all eight entry points: vsd_add_noise / vsd_lcm_step (coefficients by value, one image),
// the _frames forms (coefficients in device memory PER IMAGE of the launch, either noise source: per-frame options), the _dev forms (coefficients in device memory, a batch per launch: a captured graph follows a new strength by rewriting the floats)
// and the _seeded forms (the noise table replaced by per-image seeds in device memory: a captured graph follows a new seed per frame
// with an 8-byte copy per image, nothing re-captured).  The normal draws of a frame are a pure function of (seed, kind, draw, pixel,
// channel) -- Philox4x32-10, one block per latent pixel = its four channels, Box-Muller in fp32 -- evaluated in the thread that uses
// them; vsd_noise_fill writes a draw out (the table layout, or the raw integers).
// Launch-bound (at most batch * hw = 5 * 4096 threads at 512 x 512): 10 fixed rounds of two 32 x 32 -> 64 multiplies (a v_mul_lo_u32 /
// v_mul_hi_u32 pair each, quarter rate), no data-dependent trip count, one thread per pixel.
#include <stdarg.h>

#include "common.h"

// The bits of every frame are these kernels' fp32 operations, so the source states each one: nothing in this file is contracted by the
// compiler, and an fma is written where the contract has one.
#pragma clang fp contract(off)

namespace {

struct Philox4 {
  uint32_t x[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// ((x >> 9) + 0.5) * 2^-23: every step exact in fp32, never 0 or 1
__device__ __forceinline__ float philox_u01(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

struct Normal4 {
  float z[4];
};

// the four channels of pixel i of draw (seed, kind, d): what all three entry points share
__device__ __forceinline__ Normal4 seeded_normals(uint32_t seed_lo, uint32_t seed_hi, uint32_t kind, uint32_t d, uint32_t i, Philox4* raw = nullptr) {
  const Philox4 p = philox4x32_10(i, d, kind, 0u, seed_lo, seed_hi);
  if (raw) *raw = p;
  Normal4 n;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float r = sqrtf(-2.0f * logf(philox_u01(p.x[2 * h])));
    float s, c;
    sincosf(6.283185307179586f * philox_u01(p.x[2 * h + 1]), &s, &c);
    n.z[2 * h] = __fmul_rn(r, c);
    n.z[2 * h + 1] = __fmul_rn(r, s);
  }
  return n;
}

__global__ void noise_fill_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t kind, uint32_t draw, int hw, int raw, void* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hw) return;
  Philox4 p;
  const Normal4 n = seeded_normals(seed_lo, seed_hi, kind, draw, (uint32_t)i, &p);
  if (raw) {
    reinterpret_cast<uint4*>(out)[i] = make_uint4(p.x[0], p.x[1], p.x[2], p.x[3]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) reinterpret_cast<float*>(out)[(size_t)c * hw + i] = n.z[c];
  }
}

// Where a pixel's four normals come from: the fp32 [4][hw] table every image of the launch shares, or the image's seed.
struct TableNoise {
  const float* __restrict__ table;
  __device__ Normal4 operator()(int hw, uint32_t, uint32_t i) const {
    return Normal4{{table[i], table[(size_t)hw + i], table[(size_t)2 * hw + i], table[(size_t)3 * hw + i]}};
  }
};

struct SeededNoise {
  const uint32_t* __restrict__ seeds;  // [batch][2] = (low, high)
  uint32_t kind, draw;
  __device__ Normal4 operator()(int, uint32_t image, uint32_t i) const { return seeded_normals(seeds[2 * image], seeds[2 * image + 1], kind, draw, i); }
};

// Where the coefficients {sa, sb, cskip, cout, sap, sbp} come from: the first N of them by value (add_noise takes two, a step six),
// floats in device memory (`const float*`; add_noise reads the first two alone), or floats in device memory PER IMAGE of the launch
// (FrameCoef: image b reads base + b * stride).  coef_of(source, image) is what the bodies index; the first two ignore the image.
template <int N>
struct CoefValues {
  float v[N];
  __device__ float operator[](int j) const { return v[j]; }
};
struct FrameCoef {
  const float* __restrict__ base;
  int stride;  // floats between two images' coefficients
};
template <int N>
__device__ __forceinline__ const CoefValues<N>& coef_of(const CoefValues<N>& k, uint32_t) { return k; }
__device__ __forceinline__ const float* coef_of(const float* k, uint32_t) { return k; }
__device__ __forceinline__ const float* coef_of(const FrameCoef& k, uint32_t image) { return k.base + (size_t)image * k.stride; }

// THE SCHEDULER ARITHMETIC, per channel 0..3 in fp32 (channels 4..7 are written as zero); blockIdx.y = image of the launch:
//   out = fp16(fma(sa, x, sb * n))
template <class Noise, class Coef>
__global__ void add_noise_kernel(const half_t* __restrict__ x0, Noise noise, Coef coef, int hw, half_t* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hw) return;
  const auto& k = coef_of(coef, blockIdx.y);
  const float sa = k[0], sb = k[1];
  const Normal4 nz = noise(hw, blockIdx.y, (uint32_t)i);
  const size_t row = (size_t)blockIdx.y * hw + i;
  half8 x = *reinterpret_cast<const half8*>(x0 + row * 8);
  half8 o = (half8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = (half_t)__builtin_fmaf(sa, (float)x[c], sb * nz.z[c]);
  *reinterpret_cast<half8*>(out + row * 8) = o;
}

//   px0 = fma(-sb, e, xs) / sa;  d = fma(cskip, xs, cout * px0);  den = fp16(d);
//   prev = fp16(sap * d + sbp * n) as mul, mul, add (NOISE = false, the step that adds none: prev = den);  dec_in = fp16(tanhf(den / 3) * 3)
template <bool NOISE, class Noise, class Coef>
__global__ void lcm_step_kernel(const half_t* __restrict__ eps, const half_t* __restrict__ sample, Noise noise, Coef coef, int hw,
                                half_t* __restrict__ prev, half_t* __restrict__ den, half_t* __restrict__ dec_in) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hw) return;
  const auto& k = coef_of(coef, blockIdx.y);
  const float sa = k[0], sb = k[1], cskip = k[2], cout = k[3], sap = k[4], sbp = k[5];
  Normal4 nz = {{0.f, 0.f, 0.f, 0.f}};
  if (NOISE) nz = noise(hw, blockIdx.y, (uint32_t)i);
  const size_t row = (size_t)blockIdx.y * hw + i;
  half8 e = *reinterpret_cast<const half8*>(eps + row * 8);
  half8 x = *reinterpret_cast<const half8*>(sample + row * 8);
  half8 op = (half8){0, 0, 0, 0, 0, 0, 0, 0}, od = op, oi = op;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float xs = (float)x[c];
    float px0 = __builtin_fmaf(-sb, (float)e[c], xs) / sa;
    float d = __builtin_fmaf(cskip, xs, cout * px0);
    asm volatile("" : "+v"(d));  // d exists in fp32 before it is rounded to fp16: no v_fma_mixlo_f16 (emits nothing)
    od[c] = (half_t)d;
    float pv = NOISE ? sap * d + sbp * nz.z[c] : d;
    op[c] = (half_t)pv;
    oi[c] = (half_t)(tanhf((float)od[c] / 3.0f) * 3.0f);
  }
  if (prev) *reinterpret_cast<half8*>(prev + row * 8) = op;
  if (den) *reinterpret_cast<half8*>(den + row * 8) = od;
  if (dec_in) *reinterpret_cast<half8*>(dec_in + row * 8) = oi;
}

template <class Noise, class Coef>
void launch_add_noise(hipStream_t s, const void* x0, Noise noise, Coef k, int hw, int batch, void* out) {
  hipLaunchKernelGGL((add_noise_kernel<Noise, Coef>), dim3(cdiv(hw, 256), batch), dim3(256), 0, s, (const half_t*)x0, noise, k, hw, (half_t*)out);
}

template <class Noise, class Coef>
void launch_lcm_step(hipStream_t s, const void* eps, const void* sample, bool noisy, Noise noise, Coef k, int hw, int batch, void* prev,
                     void* den, void* dec_in) {
  auto kernel = noisy ? lcm_step_kernel<true, Noise, Coef> : lcm_step_kernel<false, Noise, Coef>;
  hipLaunchKernelGGL(kernel, dim3(cdiv(hw, 256), batch), dim3(256), 0, s, (const half_t*)eps, (const half_t*)sample, noise, k, hw, (half_t*)prev,
                     (half_t*)den, (half_t*)dec_in);
}

}  // namespace

extern "C" int vsd_noise_fill(vsd_ctx* ctx, uint32_t seed_lo, uint32_t seed_hi, int kind, int draw, int hw, int raw, void* out, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!out || hw <= 0 || kind < 0 || draw < 0 || (raw != 0 && raw != 1) || ((uintptr_t)out & (raw ? 15 : 3)))
    return vsd_fail(ctx, VSD_ERR_ARG, "noise_fill: bad arguments (hw >= 1, kind >= 0, draw >= 0, raw 0 or 1, out aligned to %d bytes)", raw ? 16 : 4);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(noise_fill_kernel, dim3(cdiv(hw, 256)), dim3(256), 0, s, seed_lo, seed_hi, (uint32_t)kind, (uint32_t)draw, hw, raw, out);
  return ls.finish();
}

extern "C" int vsd_add_noise(vsd_ctx* ctx, const void* x0, const void* noise_f32, float sqrt_a, float sqrt_b, int hw,
                             void* out, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!x0 || !noise_f32 || !out || hw <= 0) return vsd_fail(ctx, VSD_ERR_ARG, "add_noise: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  launch_add_noise(s, x0, TableNoise{(const float*)noise_f32}, CoefValues<2>{{sqrt_a, sqrt_b}}, hw, 1, out);
  return ls.finish();
}

extern "C" int vsd_lcm_step(vsd_ctx* ctx, const void* eps, const void* sample, const void* noise_f32,
                            const float* coef_host, int hw, void* prev, void* denoised, void* dec_in, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!eps || !sample || !coef_host || hw <= 0) return vsd_fail(ctx, VSD_ERR_ARG, "lcm_step: bad arguments");
  CoefValues<6> k = {{coef_host[0], coef_host[1], coef_host[2], coef_host[3], coef_host[4], coef_host[5]}};
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  launch_lcm_step(s, eps, sample, noise_f32 != nullptr, TableNoise{(const float*)noise_f32}, k, hw, 1, prev, denoised, dec_in);
  return ls.finish();
}

extern "C" int vsd_add_noise_dev(vsd_ctx* ctx, const void* x0, const void* noise_f32, const void* coef_dev, int hw, int batch,
                                 void* out, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!x0 || !noise_f32 || !coef_dev || !out || hw <= 0 || batch < 1 || batch > 65535)
    return vsd_fail(ctx, VSD_ERR_ARG, "add_noise_dev: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  launch_add_noise(s, x0, TableNoise{(const float*)noise_f32}, (const float*)coef_dev, hw, batch, out);
  return ls.finish();
}

extern "C" int vsd_lcm_step_dev(vsd_ctx* ctx, const void* eps, const void* sample, const void* noise_f32, const void* coef_dev,
                                int hw, int batch, void* prev, void* denoised, void* dec_in, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!eps || !sample || !coef_dev || hw <= 0 || batch < 1 || batch > 65535)
    return vsd_fail(ctx, VSD_ERR_ARG, "lcm_step_dev: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  launch_lcm_step(s, eps, sample, noise_f32 != nullptr, TableNoise{(const float*)noise_f32}, (const float*)coef_dev, hw, batch, prev, denoised,
                  dec_in);
  return ls.finish();
}

extern "C" int vsd_add_noise_seeded(vsd_ctx* ctx, const void* x0, const void* seeds_dev, int kind, int draw, const void* coef_dev, int hw, int batch,
                                    void* out, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!x0 || !seeds_dev || !coef_dev || !out || hw <= 0 || batch < 1 || batch > 65535 || kind < 0 || draw < 0)
    return vsd_fail(ctx, VSD_ERR_ARG, "add_noise_seeded: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  launch_add_noise(s, x0, SeededNoise{(const uint32_t*)seeds_dev, (uint32_t)kind, (uint32_t)draw}, (const float*)coef_dev, hw, batch, out);
  return ls.finish();
}

extern "C" int vsd_lcm_step_seeded(vsd_ctx* ctx, const void* eps, const void* sample, const void* seeds_dev, int kind, int draw, const void* coef_dev,
                                   int hw, int batch, void* prev, void* denoised, void* dec_in, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!eps || !sample || !coef_dev || hw <= 0 || batch < 1 || batch > 65535 || kind < 0 || (draw > 0 && !seeds_dev))
    return vsd_fail(ctx, VSD_ERR_ARG, "lcm_step_seeded: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  launch_lcm_step(s, eps, sample, draw > 0, SeededNoise{(const uint32_t*)seeds_dev, (uint32_t)kind, (uint32_t)draw}, (const float*)coef_dev, hw, batch,
                  prev, denoised, dec_in);
  return ls.finish();
}

// ---- coefficients per image of the launch (include/vsd.h: per-frame options): the same two bodies, the coefficient source indexed by image
extern "C" int vsd_add_noise_frames(vsd_ctx* ctx, const void* x0, const void* noise_f32, const void* seeds_dev, int kind, int draw,
                                    const void* coef_dev, int coef_stride, int hw, int batch, void* out, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!x0 || !coef_dev || !out || hw <= 0 || batch < 1 || batch > 65535 || coef_stride < 2 || ((uintptr_t)coef_dev & 3))
    return vsd_fail(ctx, VSD_ERR_ARG, "add_noise_frames: bad arguments (hw >= 1, batch 1..65535, coef_stride >= 2)");
  if ((noise_f32 != nullptr) == (seeds_dev != nullptr))
    return vsd_fail(ctx, VSD_ERR_ARG, "add_noise_frames: exactly one of noise_f32 and seeds_dev must be given");
  if (seeds_dev && (kind < 0 || draw < 0)) return vsd_fail(ctx, VSD_ERR_ARG, "add_noise_frames: kind=%d draw=%d", kind, draw);
  hipStream_t s = (hipStream_t)stream;
  const FrameCoef k{(const float*)coef_dev, coef_stride};
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  if (noise_f32)
    launch_add_noise(s, x0, TableNoise{(const float*)noise_f32}, k, hw, batch, out);
  else
    launch_add_noise(s, x0, SeededNoise{(const uint32_t*)seeds_dev, (uint32_t)kind, (uint32_t)draw}, k, hw, batch, out);
  return ls.finish();
}

extern "C" int vsd_lcm_step_frames(vsd_ctx* ctx, const void* eps, const void* sample, const void* noise_f32, const void* seeds_dev, int kind,
                                   int draw, const void* coef_dev, int coef_stride, int hw, int batch, void* prev, void* denoised, void* dec_in,
                                   void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!eps || !sample || !coef_dev || hw <= 0 || batch < 1 || batch > 65535 || coef_stride < 6 || ((uintptr_t)coef_dev & 3))
    return vsd_fail(ctx, VSD_ERR_ARG, "lcm_step_frames: bad arguments (hw >= 1, batch 1..65535, coef_stride >= 6)");
  if (noise_f32 && seeds_dev) return vsd_fail(ctx, VSD_ERR_ARG, "lcm_step_frames: at most one of noise_f32 and seeds_dev may be given");
  if (seeds_dev && (kind < 0 || draw < 1)) return vsd_fail(ctx, VSD_ERR_ARG, "lcm_step_frames: seeded noise needs kind >= 0 and draw >= 1, got %d, %d", kind, draw);
  hipStream_t s = (hipStream_t)stream;
  const FrameCoef k{(const float*)coef_dev, coef_stride};
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  if (seeds_dev)
    launch_lcm_step(s, eps, sample, true, SeededNoise{(const uint32_t*)seeds_dev, (uint32_t)kind, (uint32_t)draw}, k, hw, batch, prev, denoised, dec_in);
  else
    launch_lcm_step(s, eps, sample, noise_f32 != nullptr, TableNoise{(const float*)noise_f32}, k, hw, batch, prev, denoised, dec_in);
  return ls.finish();
}

// ---- the latent anchor of a keep mask (include/vsd.h THE KEEP MASK): beside the bodies above because it reads their noise and coefficient
// sources.  Per channel 0..3 in fp32 (channels 4..7 stay as they are); blockIdx.y = image of the launch; a row whose weight is 1 is not written:
//   step:  kept = fma(sap, x0, sbp * n0);  lat = fp16(fma(wl, lat, (1 - wl) * kept))
//   final: den = fp16(fma(wl, den, (1 - wl) * x0));  dec_in = fp16(tanhf(den / 3) * 3), lcm_step_kernel's expression, for every row
namespace {

__device__ __host__ __forceinline__ float keep_blend(float wl, float mine, float kept) { return __builtin_fmaf(wl, mine, (1.0f - wl) * kept); }
__device__ __host__ __forceinline__ float keep_noised(float sap, float x, float sbp, float n) { return __builtin_fmaf(sap, x, sbp * n); }

template <class Noise, class Coef>
__global__ void latent_keep_step_kernel(const half_t* __restrict__ x0, const float* __restrict__ weights, Noise noise, Coef coef, int hw,
                                        half_t* __restrict__ lat) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hw) return;
  const size_t row = (size_t)blockIdx.y * hw + i;
  const float wl = weights[row];
  if (wl == 1.0f) return;
  const auto& k = coef_of(coef, blockIdx.y);
  const float sap = k[4], sbp = k[5];
  const Normal4 nz = noise(hw, blockIdx.y, (uint32_t)i);
  half8 x = *reinterpret_cast<const half8*>(x0 + row * 8);
  half8 l = *reinterpret_cast<const half8*>(lat + row * 8);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float v = keep_blend(wl, (float)l[c], keep_noised(sap, (float)x[c], sbp, nz.z[c]));
    asm volatile("" : "+v"(v));  // v exists in fp32 before it is rounded to fp16: no v_fma_mixlo_f16 (emits nothing)
    l[c] = (half_t)v;
  }
  *reinterpret_cast<half8*>(lat + row * 8) = l;
}

__global__ void latent_keep_final_kernel(const half_t* __restrict__ x0, const float* __restrict__ weights, int hw, half_t* __restrict__ den,
                                         half_t* __restrict__ dec_in) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hw) return;
  const size_t row = (size_t)blockIdx.y * hw + i;
  const float wl = weights[row];
  half8 d = *reinterpret_cast<const half8*>(den + row * 8);
  half8 oi = (half8){0, 0, 0, 0, 0, 0, 0, 0};
  if (wl != 1.0f) {
    half8 x = *reinterpret_cast<const half8*>(x0 + row * 8);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = keep_blend(wl, (float)d[c], (float)x[c]);
      asm volatile("" : "+v"(v));
      d[c] = (half_t)v;
    }
    *reinterpret_cast<half8*>(den + row * 8) = d;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) oi[c] = (half_t)(tanhf((float)d[c] / 3.0f) * 3.0f);
  *reinterpret_cast<half8*>(dec_in + row * 8) = oi;
}

template <class Noise, class Coef>
void launch_latent_keep(hipStream_t s, const void* x0, const void* weights, Noise noise, Coef k, int hw, int batch, void* lat) {
  hipLaunchKernelGGL((latent_keep_step_kernel<Noise, Coef>), dim3(cdiv(hw, 256), batch), dim3(256), 0, s, (const half_t*)x0, (const float*)weights, noise,
                     k, hw, (half_t*)lat);
}

template <class Noise>
void launch_latent_keep(hipStream_t s, const void* x0, const void* weights, Noise noise, const void* coef_dev, int coef_stride, int hw, int batch,
                        void* lat) {
  if (coef_stride)
    launch_latent_keep(s, x0, weights, noise, FrameCoef{(const float*)coef_dev, coef_stride}, hw, batch, lat);
  else
    launch_latent_keep(s, x0, weights, noise, (const float*)coef_dev, hw, batch, lat);
}

}  // namespace

extern "C" int vsd_latent_keep(vsd_ctx* ctx, const void* x0, const void* weights_f32, const void* noise_f32, const void* seeds_dev, int kind, int draw,
                               const void* coef_dev, int coef_stride, int hw, int batch, void* lat, void* den, void* dec_in, void* stream) {
  if (!ctx) return VSD_ERR_ARG;
  if (!x0 || !weights_f32 || hw <= 0 || batch < 1 || batch > 65535 || ((uintptr_t)weights_f32 & 3))
    return vsd_fail(ctx, VSD_ERR_ARG, "latent_keep: bad arguments (x0, weights_f32 4-byte aligned, hw >= 1, batch 1..65535)");
  hipStream_t s = (hipStream_t)stream;
  if (lat) {  // the step form
    if (den || dec_in) return vsd_fail(ctx, VSD_ERR_ARG, "latent_keep: the step form (lat given) takes neither den nor dec_in");
    if ((noise_f32 != nullptr) == (seeds_dev != nullptr))
      return vsd_fail(ctx, VSD_ERR_ARG, "latent_keep: the step form needs exactly one of noise_f32 and seeds_dev");
    if (!coef_dev || ((uintptr_t)coef_dev & 3) || (coef_stride != 0 && coef_stride < 6))
      return vsd_fail(ctx, VSD_ERR_ARG, "latent_keep: the step form needs coef_dev (4-byte aligned) and coef_stride 0 or >= 6, got %d", coef_stride);
    if (seeds_dev && (kind < 0 || draw < 0)) return vsd_fail(ctx, VSD_ERR_ARG, "latent_keep: kind=%d draw=%d", kind, draw);
    LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
    if (noise_f32)
      launch_latent_keep(s, x0, weights_f32, TableNoise{(const float*)noise_f32}, coef_dev, coef_stride, hw, batch, lat);
    else
      launch_latent_keep(s, x0, weights_f32, SeededNoise{(const uint32_t*)seeds_dev, (uint32_t)kind, (uint32_t)draw}, coef_dev, coef_stride, hw, batch, lat);
    return ls.finish();
  }
  if (!den || !dec_in) return vsd_fail(ctx, VSD_ERR_ARG, "latent_keep: give lat (the step form) or den and dec_in (the final form)");
  if (noise_f32 || seeds_dev) return vsd_fail(ctx, VSD_ERR_ARG, "latent_keep: the final form (den, dec_in) takes no noise source");
  LaunchScope ls(ctx, s, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(latent_keep_final_kernel, dim3(cdiv(hw, 256), batch), dim3(256), 0, s, (const half_t*)x0, (const float*)weights_f32, hw, (half_t*)den,
                     (half_t*)dec_in);
  return ls.finish();
}

// The anchor as plain host loops over HOST memory (no context): table noise only, writes lat (step form) or den (final form) only --
// the host's tanhf is not the device's, so there is no dec_in here.  coef: image b reads sap, sbp at coef[b * coef_stride + 4], [.. + 5].
extern "C" int vsd_latent_keep_host(const void* x0, const float* weights_f32, const float* noise_f32, const float* coef, int coef_stride, int hw,
                                    int batch, void* lat, void* den) {
  if (!x0 || !weights_f32 || hw <= 0 || batch < 1 || batch > 65535) return VSD_ERR_ARG;
  const bool step = lat != nullptr;
  if (step ? (den || !noise_f32 || !coef || (coef_stride != 0 && coef_stride < 6)) : (!den || noise_f32)) return VSD_ERR_ARG;
  const half_t* x = (const half_t*)x0;
  half_t* out = (half_t*)(step ? lat : den);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < hw; ++i) {
      const size_t row = (size_t)b * hw + i;
      const float wl = weights_f32[row];
      if (wl == 1.0f) continue;
      for (int c = 0; c < 4; ++c) {
        const float xc = (float)x[row * 8 + c];
        const float kept = step ? keep_noised(coef[(size_t)b * coef_stride + 4], xc, coef[(size_t)b * coef_stride + 5], noise_f32[(size_t)c * hw + i]) : xc;
        const volatile float v = keep_blend(wl, (float)out[row * 8 + c], kept);  // (rounded to fp32 first, as on the device)
        out[row * 8 + c] = (half_t)v;
      }
    }
  return VSD_OK;
}
