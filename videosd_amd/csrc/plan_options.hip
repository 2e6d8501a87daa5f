// vsd_plan_set_options on the device: the option-dependent constants of a loaded plan (videosd_amd/plan.py, LIVE OPTIONS) rewritten
// by ONE launch on the plan's stream -- what Engine._write_constants does with uploads and the ~10 GEMMs of the time path.  Everything
// a schedule needs was computed at export, per timestep; this only picks rows: grid (x, step, table) copies row[step] of each 50-row
// time table into the table the captured graph reads, and workgroup (0, 0, 0) writes the fp32 constant block from the coefficient
// table.  The step -> row indices and the scale travel in the argument block: nothing to upload, nothing to wait for.
#include <stdarg.h>
#include <algorithm>

#include "plan_options.h"

namespace {

constexpr int OPT_THREADS = 256;

__global__ __launch_bounds__(OPT_THREADS) void plan_options_kernel(const PlanOptArgs a) {
  const int step = blockIdx.y;
  const PlanOptTable t = a.tab[blockIdx.z];
  const uint32_t* src = t.src + (size_t)a.row[step] * t.row_words;
  uint32_t* dst = t.dst + (size_t)step * t.dst_stride_words;
  for (uint32_t w = blockIdx.x * OPT_THREADS + threadIdx.x; w < t.row_words; w += gridDim.x * OPT_THREADS) dst[w] = src[w];
  if (blockIdx.x | blockIdx.y | blockIdx.z) return;
  const int ncoef = 2 + PLAN_OPT_COEF * a.n;
  for (int i = threadIdx.x; i < ncoef + a.nres; i += OPT_THREADS) {
    float v;
    if (i < 2) {  // add_noise at the first timestep
      v = a.coef[a.row[0] * PLAN_OPT_COEF + 4 + i];
    } else if (i < ncoef) {
      const int s = (i - 2) / PLAN_OPT_COEF, k = (i - 2) % PLAN_OPT_COEF;
      // [4], [5]: sqrt(a), sqrt(1 - a) of the NEXT timestep (the last step: its own), lcm.LCMSchedule.step_coef
      const int r = k < 4 ? a.row[s] : a.row[s + 1 < a.n ? s + 1 : s];
      v = a.coef[r * PLAN_OPT_COEF + (k < 4 ? k : k - 4)];
    } else {
      // logspace[k] * (float)scale as ONE fp32 multiply, as torch computes it on the host: no contraction, no reassociation
      v = __fmul_rn(a.coef[PLAN_OPT_ROWS * PLAN_OPT_COEF + (i - ncoef)], a.scale);
    }
    a.consts[i] = v;
  }
}

}  // namespace

int plan_options_launch(vsd_ctx* ctx, hipStream_t stream, const PlanOptArgs& a) {
  if (a.n < 1 || a.n > PLAN_OPT_ROWS || a.ntab < 1 || a.ntab > PLAN_OPT_TABLES || a.nres < 0) return vsd_fail(ctx, VSD_ERR_ARG, "plan_set_options: bad option tables");
  uint32_t words = 0;
  for (int t = 0; t < a.ntab; ++t) words = a.tab[t].row_words > words ? a.tab[t].row_words : words;
  const int gx = std::max(1, std::min(16, cdiv((int)words, 4 * OPT_THREADS)));
  LaunchScope ls(ctx, stream, VSD_FAM_ELEMENTWISE, 0.0);
  hipLaunchKernelGGL(plan_options_kernel, dim3(gx, a.n, a.ntab), dim3(OPT_THREADS), 0, stream, a);
  return ls.finish();
}
