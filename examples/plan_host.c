/* A host WITHOUT Python driving frames through the denoising path (include/vsd.h vsd_plan_*): what SURVEY.md section 8b's
 * whole-frame entry points are for.  The plan file comes from videosd_amd.plan.export_plan / VideoSDPipeline.export_plan (one frame
 * size / step count / prompt / frames per launch).
 *
 *   gcc -O2 examples/plan_host.c -Iinclude -Lvideosd_amd -lvsd -Wl,-rpath,$PWD/videosd_amd -o /tmp/plan_host
 *   /tmp/plan_host [--seed N] frame.vsdplan in.raw out.raw [launches] [lanes] [strength controlnet_scale]
 * in.raw / out.raw: uint8 [frames per launch][H][W][3].  lanes (1..4): that many plans of the program in flight, one per launch
 * stream (the reference keeps N actors per node, server.py:132-137; inside one process the launch lanes do the same) -- frame k goes
 * to lane k mod lanes.  The file is read ONCE: lane 0 loads it, the other lanes are clones that share its weights on the device
 * (vsd_plan_clone_lane).  strength controlnet_scale: the reference's live options (server.py:163-197), applied to every lane with
 * vsd_plan_set_options before the timed loop.  --seed N (anywhere on the line; a plan exported with device_seed only): every frame of
 * every launch is denoised with the noise of seed N (vsd_plan_set_seeds; the client's seed box, server.py:181-182).  Prints the frame
 * rate; out.raw is lane 0's last result.
 * (the reference's caller is a Python loop, server.py:104-143; this is that loop for a C / C++ / Go-via-cgo media server) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "vsd.h"

int main(int argc, char** argv) {
  int have_seed = 0;
  uint64_t seed = 0;
  for (int i = 1; i + 1 < argc; ++i)
    if (strcmp(argv[i], "--seed") == 0) {  /* taken out of the line: the positional arguments keep their places */
      have_seed = 1;
      seed = strtoull(argv[i + 1], NULL, 0);
      memmove(argv + i, argv + i + 2, (size_t)(argc - i - 2) * sizeof(char*));
      argc -= 2;
      break;
    }
  if (argc < 4) {
    fprintf(stderr, "usage: %s [--seed N] plan in.raw out.raw [launches] [lanes] [strength controlnet_scale]\n", argv[0]);
    return 2;
  }
  const int launches = argc > 4 ? atoi(argv[4]) : 1;
  int lanes = argc > 5 ? atoi(argv[5]) : 1;
  if (lanes < 1 || lanes > VSD_POOL_STREAMS) lanes = 1;
  vsd_ctx* ctx = vsd_create(0);
  if (!ctx) { fprintf(stderr, "no HIP device\n"); return 1; }
  vsd_plan* plan[VSD_POOL_STREAMS];
  unsigned char *in[VSD_POOL_STREAMS], *out[VSD_POOL_STREAMS];
  int dims[3];
  size_t n = 0;
  for (int l = 0; l < lanes; ++l) {
    /* one lane: a stream of the plan's own; several: the process's launch streams (own hardware queues, vsd_stream_pool), lane 0 from
     * the file and the others cloned from it */
    const int rc = lanes == 1 ? vsd_plan_load(ctx, argv[1], &plan[l])
                   : l == 0   ? vsd_plan_load_lane(ctx, argv[1], 0, &plan[0])
                              : vsd_plan_clone_lane(ctx, plan[0], l, &plan[l]);
    if (rc != VSD_OK) { fprintf(stderr, "%s\n", vsd_last_error(ctx)); return 1; }
    if (argc > 7) {
      const int orc = vsd_plan_set_options(ctx, plan[l], atof(argv[6]), atof(argv[7]));
      if (orc == VSD_PLAN_OTHER_PROGRAM) { fprintf(stderr, "strength %s needs another number of steps than this plan has: export another plan\n", argv[6]); return 1; }
      if (orc != VSD_OK) { fprintf(stderr, "%s\n", vsd_last_error(ctx)); return 1; }
    }
    vsd_plan_info(ctx, plan[l], dims);
    if (have_seed) {  /* one seed per frame of the launch; stream-ordered like the options */
      uint64_t seeds[1024];
      for (int b = 0; b < dims[2] && b < 1024; ++b) seeds[b] = seed;
      if (vsd_plan_set_seeds(ctx, plan[l], seeds, dims[2]) != VSD_OK) { fprintf(stderr, "%s\n", vsd_last_error(ctx)); return 1; }
    }
    n = (size_t)dims[2] * dims[0] * dims[1] * 3;
    in[l] = vsd_pinned_alloc(ctx, n);
    out[l] = vsd_pinned_alloc(ctx, n);
    if (!in[l] || !out[l]) { fprintf(stderr, "no pinned host memory\n"); return 1; }
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(in[0], 1, n, f) != n) { fprintf(stderr, "%s: need %zu bytes (%d x %d x %d x 3)\n", argv[2], n, dims[2], dims[0], dims[1]); return 1; }
  fclose(f);
  for (int l = 1; l < lanes; ++l) memcpy(in[l], in[0], n);
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (int i = 0; i < launches; ++i) {
    const int l = i % lanes;
    if (i >= lanes && vsd_plan_wait(ctx, plan[l]) != VSD_OK) { fprintf(stderr, "%s\n", vsd_last_error(ctx)); return 1; }  /* the lane's previous frame */
    if (vsd_plan_submit(ctx, plan[l], in[l], out[l]) != VSD_OK) { fprintf(stderr, "%s\n", vsd_last_error(ctx)); return 1; }
  }
  for (int l = 0; l < lanes; ++l)
    if (vsd_plan_wait(ctx, plan[l]) != VSD_OK) { fprintf(stderr, "%s\n", vsd_last_error(ctx)); return 1; }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  const double s = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out[0], 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
  fclose(f);
  printf("%d x %d, %d frame(s) per launch, %d lane(s): %d launches in %.3f s = %.1f frames/s, %.2f ms per launch per lane\n", dims[1], dims[0], dims[2], lanes,
         launches, s, launches * dims[2] / s, 1e3 * s / launches * lanes);
  for (int l = 0; l < lanes; ++l) {
    vsd_plan_free(ctx, plan[l]);
    vsd_pinned_free(ctx, in[l]);
    vsd_pinned_free(ctx, out[l]);
  }
  vsd_destroy(ctx);
  return 0;
}
