/* A host WITHOUT Python feeding CAMERA frames of any size to a plan (include/vsd.h vsd_plan_infer_frame): the centre crop and the
 * LANCZOS resize the reference does with PIL in front of every frame (videopipeline.py:92-107) run on the GPU, bit for bit Pillow's,
 * so this program returns the picture VideoSDPipeline.infer returns for the same frame.  The plan file comes from
 * videosd_amd.plan.export_plan / VideoSDPipeline.export_plan (examples/plan_host.c feeds frames that already have the plan's size).
 *
 *   gcc -O2 examples/camera_host.c -Iinclude -Lvideosd_amd -lvsd -Wl,-rpath,$PWD/videosd_amd -o /tmp/camera_host
 *   /tmp/camera_host frame.vsdplan camera.raw width height out.raw [launches] [i420]
 * camera.raw: uint8 [frames per launch][height][width][3], any width and height; out.raw: uint8 [frames per launch][H][W][3] of the plan.
 * With a trailing `i420` (the frames of a WebRTC loop, vsd_plan_infer_frame_i420): camera.raw is raw planar YUV 4:2:0 -- all Y planes
 * ([frames per launch][height][width]), then all U, then all V planes ([frames per launch][ceil(height / 2)][ceil(width / 2)]) -- and
 * out.raw is packed I420, H * W * 3 / 2 bytes per frame; the colour conversion runs on the GPU both ways (contract: include/vsd.h). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "vsd.h"

int main(int argc, char** argv) {
  const int i420 = argc > 6 && strcmp(argv[argc - 1], "i420") == 0;
  if (i420) --argc;
  if (argc < 6) {
    fprintf(stderr, "usage: %s plan camera.raw width height out.raw [launches] [i420]\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[3]), h = atoi(argv[4]);
  const int launches = argc > 6 ? atoi(argv[6]) : 1;
  if (w < 1 || h < 1 || w > VSD_RESAMPLE_MAX_SIDE || h > VSD_RESAMPLE_MAX_SIDE) { fprintf(stderr, "width and height: 1..%d\n", VSD_RESAMPLE_MAX_SIDE); return 2; }
  vsd_ctx* ctx = vsd_create(0);
  if (!ctx) { fprintf(stderr, "no HIP device\n"); return 1; }
  vsd_plan* plan = NULL;
  int dims[3], box[4];
  if (vsd_plan_load(ctx, argv[1], &plan) != VSD_OK) { fprintf(stderr, "%s\n", vsd_last_error(ctx)); return 1; }
  vsd_plan_info(ctx, plan, dims);
  const size_t n_y = (size_t)dims[2] * h * w, n_c = (size_t)dims[2] * ((h + 1) / 2) * ((w + 1) / 2);
  const size_t n_in = i420 ? n_y + 2 * n_c : n_y * 3, n_out = (size_t)dims[2] * dims[0] * dims[1] * (i420 ? 3 : 6) / 2;
  unsigned char* in = vsd_pinned_alloc(ctx, n_in);
  unsigned char* out = vsd_pinned_alloc(ctx, n_out);
  if (!in || !out) { fprintf(stderr, "no pinned host memory\n"); return 1; }
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(in, 1, n_in, f) != n_in) { fprintf(stderr, "%s: need %zu bytes (%d x %d x %d x %s)\n", argv[2], n_in, dims[2], h, w, i420 ? "1.5" : "3"); return 1; }
  fclose(f);
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (int i = 0; i < launches; ++i) {
    const int rc = i420 ? vsd_plan_infer_frame_i420(ctx, plan, in, w, in + n_y, in + n_y + n_c, (w + 1) / 2, h, w, out)
                        : vsd_plan_infer_frame(ctx, plan, in, h, w, (int64_t)3 * w, out);
    if (rc != VSD_OK) { fprintf(stderr, "%s\n", vsd_last_error(ctx)); return 1; }
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  const double s = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
  f = fopen(argv[5], "wb");
  if (!f || fwrite(out, 1, n_out, f) != n_out) { fprintf(stderr, "cannot write %s\n", argv[5]); return 1; }
  fclose(f);
  vsd_center_crop_box(w, h, dims[1], dims[0], box);
  printf("%d x %d %s camera frames, crop box (%d, %d, %d, %d) -> %d x %d, %d frame(s) per launch: %d launches in %.3f s = %.1f frames/s\n", w, h,
         i420 ? "I420" : "RGB", box[0], box[1], box[2], box[3], dims[1], dims[0], dims[2], launches, s, launches * dims[2] / s);
  vsd_plan_free(ctx, plan);
  vsd_pinned_free(ctx, in);
  vsd_pinned_free(ctx, out);
  vsd_destroy(ctx);
  return 0;
}
