// A prepared frame program from a file, for hosts without Python (include/vsd.h vsd_plan_*; format and export: videosd_amd/plan.py).
//
// SURVEY.md section 8b sketched whole-frame C entry points; a frame's sequencing lives in engine.py, so what a non-Python host gets
// is the RECORDED program: every C-ABI call of the engine's one-stream form with its arguments, device pointers as (region, offset).
// vsd_plan_load allocates the regions, uploads the saved ones (weights, constants, prompt block, counters), patches the pointers,
// replays the calls under stream capture and instantiates the graph; vsd_plan_infer = upload the frame(s), one graph launch,
// download.  Same kernels with the same arguments as the Python engine: the same bits (tests/test_plan_gpu.py).
#include <stdarg.h>
#include <algorithm>

#include "common.h"

namespace {

enum { T_I32 = 0, T_F32 = 1, T_PTR = 2, T_NULL = 3, T_STREAM = 4, T_DESC = 5 };
constexpr int PLAN_MAX_ARGS = 24;

union PlanArg {
  void* p;
  int i;
  float f;
};

struct PlanCall {
  int fn, n;
  PlanArg a[PLAN_MAX_ARGS];
};

}  // namespace

struct vsd_plan {
  vsd_ctx* ctx = nullptr;
  int H = 0, W = 0, batch = 0;
  std::vector<void*> regions;
  std::vector<std::vector<unsigned char>> blobs;  // descriptor arrays of the calls (the calls point into them: a moved vector keeps its buffer)
  std::vector<PlanCall> calls;
  hipStream_t stream = nullptr;
  bool own_stream = true;  // (a launch lane's stream belongs to the process-wide pool)
  void* graph = nullptr;
  void *in = nullptr, *out = nullptr, *prompt = nullptr;
  size_t io_bytes = 0, prompt_bytes = 0;
  // camera frames (vsd_plan_submit_frame): the uploaded crop boxes, the intermediate of the two passes and the tables of the last source size
  void *raw = nullptr, *work = nullptr, *table_x = nullptr, *table_y = nullptr;
  size_t raw_bytes = 0, work_bytes = 0;
  int table_x_in = 0, table_y_in = 0;
  // I420 camera frames (vsd_plan_submit_frame_i420): the uploaded plane rectangles and the packed I420 result
  void *yuv_in = nullptr, *yuv_out = nullptr;
  size_t yuv_in_bytes = 0, yuv_out_bytes = 0;
};

namespace {

int plan_dispatch(vsd_ctx* ctx, int fn, int n, const PlanArg* a) {
  switch (fn) {
#include "plan_dispatch.inc"
    default: return -1;
  }
}

struct Reader {
  FILE* f;
  bool ok = true;
  template <class T>
  T get() {
    T v{};
    if (ok && fread(&v, sizeof(T), 1, f) != 1) ok = false;
    return v;
  }
  bool bytes(void* dst, size_t n) {
    if (ok && n && fread(dst, 1, n, f) != n) ok = false;
    return ok;
  }
};

void plan_release(vsd_plan* p) {
  if (!p) return;
  if (p->graph) (void)hipGraphExecDestroy((hipGraphExec_t)p->graph);
  if (p->stream && p->own_stream) (void)hipStreamDestroy(p->stream);
  for (void* r : p->regions)
    if (r) (void)hipFree(r);
  for (void* r : {p->raw, p->work, p->table_x, p->table_y, p->yuv_in, p->yuv_out})
    if (r) (void)hipFree(r);
  delete p;
}

// a device buffer of the plan grown to `need` bytes (never shrunk); waits for the plan's stream first: nothing in flight reads the old one
int plan_grow(vsd_ctx* ctx, vsd_plan* plan, const char* who, void** p, size_t* have, size_t need) {
  if (*have >= need) return VSD_OK;
  VSD_HIP(ctx, hipStreamSynchronize(plan->stream));
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  if (hipMalloc(p, need) != hipSuccess) return vsd_fail(ctx, VSD_ERR_NOMEM, "%s: out of device memory (%zu bytes)", who, need);
  *have = need;
  return VSD_OK;
}

// the plan's table of one axis for another source length
int plan_table(vsd_ctx* ctx, vsd_plan* plan, const char* who, void** t, int* have_in, int in, int out) {
  if (in == out || *have_in == in) return VSD_OK;
  VSD_HIP(ctx, hipStreamSynchronize(plan->stream));
  if (*t) (void)hipFree(*t);
  *t = nullptr;
  *have_in = 0;
  if (hipMalloc(t, (size_t)vsd_resample_table_bytes(in, out)) != hipSuccess) return vsd_fail(ctx, VSD_ERR_NOMEM, "%s: out of device memory (table)", who);
  const int rc = vsd_resample_table_upload(ctx, in, out, *t, (void*)plan->stream);
  if (rc == VSD_OK) *have_in = in;
  return rc;
}

}  // namespace

extern "C" int vsd_plan_load(vsd_ctx* ctx, const char* path, vsd_plan** plan_out) { return vsd_plan_load_lane(ctx, path, -1, plan_out); }

// lane >= 0: the plan launches on launch stream `lane` of the process's pool (vsd_stream_pool: four CU-masked streams = four hardware
// queues on four command-processor pipes) -- several plans in flight side by side, as the Python workers' launch lanes
extern "C" int vsd_plan_load_lane(vsd_ctx* ctx, const char* path, int lane, vsd_plan** plan_out) {
  if (!ctx || !path || !plan_out) return VSD_ERR_ARG;
  if (lane >= VSD_POOL_STREAMS) return vsd_fail(ctx, VSD_ERR_ARG, "plan_load: lane %d (0..%d, or -1 for a stream of the plan's own)", lane, VSD_POOL_STREAMS - 1);
  *plan_out = nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) return vsd_fail(ctx, VSD_ERR_ARG, "plan_load: cannot open %s", path);
  Reader r{f};
  char magic[8];
  r.bytes(magic, 8);
  if (!r.ok || memcmp(magic, "VSDPLAN1", 8) != 0) {
    fclose(f);
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_load: %s is not a plan file", path);
  }
  const uint32_t version = r.get<uint32_t>();
  vsd_plan* p = new vsd_plan;
  p->ctx = ctx;
  p->H = (int)r.get<uint32_t>();
  p->W = (int)r.get<uint32_t>();
  p->batch = (int)r.get<uint32_t>();
  const uint32_t nreg = r.get<uint32_t>(), ncall = r.get<uint32_t>();
  const uint32_t in_r = r.get<uint32_t>();
  const uint64_t in_off = r.get<uint64_t>();
  const uint32_t out_r = r.get<uint32_t>();
  const uint64_t out_off = r.get<uint64_t>();
  const uint32_t pr_r = r.get<uint32_t>();
  const uint64_t pr_off = r.get<uint64_t>(), pr_bytes = r.get<uint64_t>();
  auto fail = [&](const char* what) {
    fclose(f);
    plan_release(p);
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_load: %s (%s)", what, path);
  };
  if (!r.ok || version != 1 || nreg == 0 || nreg > (1u << 20) || ncall == 0 || ncall > (1u << 22) || in_r >= nreg || out_r >= nreg)
    return fail("bad header");
  std::vector<uint64_t> size(nreg);
  std::vector<uint32_t> saved(nreg);
  for (uint32_t i = 0; i < nreg; ++i) {
    size[i] = r.get<uint64_t>();
    saved[i] = r.get<uint32_t>();
    (void)r.get<uint32_t>();
  }
  if (!r.ok) return fail("truncated region table");
  (void)hipSetDevice(ctx->device);
  p->regions.assign(nreg, nullptr);
  for (uint32_t i = 0; i < nreg; ++i) {
    if (hipMalloc(&p->regions[i], size[i] ? size[i] : 16) != hipSuccess) return fail("out of device memory");
    if (!saved[i] && hipMemset(p->regions[i], 0, size[i]) != hipSuccess) return fail("hipMemset failed");
  }
  if (lane >= 0) {
    void* pool[VSD_POOL_STREAMS];
    if (vsd_stream_pool(ctx, pool) != VSD_OK) return fail("no launch stream pool");
    p->stream = (hipStream_t)pool[lane];
    p->own_stream = false;
  } else if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) {
    return fail("hipStreamCreate failed");
  }
  auto at = [&](uint32_t reg, uint64_t off, void** out) {
    if (reg >= nreg || off >= size[reg]) return false;
    *out = (char*)p->regions[reg] + off;
    return true;
  };
  p->calls.resize(ncall);
  for (uint32_t c = 0; c < ncall; ++c) {
    PlanCall& pc = p->calls[c];
    pc.fn = (int)r.get<uint32_t>();
    pc.n = (int)r.get<uint32_t>();
    if (!r.ok || pc.n < 0 || pc.n > PLAN_MAX_ARGS) return fail("bad call record");
    for (int k = 0; k < pc.n; ++k) {
      const uint32_t tag = r.get<uint32_t>(), aux = r.get<uint32_t>();
      const uint64_t val = r.get<uint64_t>();
      if (!r.ok) return fail("truncated call list");
      pc.a[k].p = nullptr;
      switch (tag) {
        case T_I32: pc.a[k].i = (int)(int64_t)val; break;
        case T_F32: { const uint32_t b = (uint32_t)val; memcpy(&pc.a[k].f, &b, 4); break; }
        case T_PTR: if (!at(aux, val, &pc.a[k].p)) return fail("pointer outside its region"); break;
        case T_NULL: break;
        case T_STREAM: pc.a[k].p = (void*)p->stream; break;
        case T_DESC: {
          if (aux == 0 || aux > VSD_CONV_GROUP_MAX || val != (uint64_t)aux * sizeof(vsd_conv_desc)) return fail("descriptor array of another interface version");
          p->blobs.emplace_back((size_t)val);
          std::vector<unsigned char>& blob = p->blobs.back();
          r.bytes(blob.data(), blob.size());
          const uint32_t nfix = r.get<uint32_t>();
          if (!r.ok || nfix > 64 * aux) return fail("bad descriptor record");
          for (uint32_t j = 0; j < nfix; ++j) {
            const uint32_t boff = r.get<uint32_t>(), reg = r.get<uint32_t>();
            const uint64_t off = r.get<uint64_t>();
            void* q = nullptr;
            if (!r.ok || boff + sizeof(void*) > blob.size() || !at(reg, off, &q)) return fail("bad descriptor pointer");
            memcpy(blob.data() + boff, &q, sizeof(void*));
          }
          pc.a[k].p = blob.data();
          break;
        }
        default: return fail("unknown argument tag");
      }
    }
  }
  for (uint32_t i = 0; i < nreg; ++i) {
    if (!saved[i]) continue;
    std::vector<unsigned char> host(1 << 24);
    uint64_t done = 0;
    while (done < size[i]) {
      const size_t n = (size_t)std::min<uint64_t>(host.size(), size[i] - done);
      if (!r.bytes(host.data(), n)) return fail("truncated region contents");
      if (hipMemcpy((char*)p->regions[i] + done, host.data(), n, hipMemcpyHostToDevice) != hipSuccess) return fail("upload failed");
      done += n;
    }
  }
  fclose(f);
  f = nullptr;
  if (!at(in_r, in_off, &p->in) || !at(out_r, out_off, &p->out) || !at(pr_r, pr_off, &p->prompt) || pr_off + pr_bytes > size[pr_r]) {
    plan_release(p);
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_load: frame buffers / prompt block outside their regions");
  }
  p->prompt_bytes = (size_t)pr_bytes;
  p->io_bytes = (size_t)p->batch * p->H * p->W * 3;
  // one eager pass (first-touch of every kernel, the error reports of the ops), then the captured one
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      int rc = vsd_graph_begin(ctx, (void*)p->stream);
      if (rc != VSD_OK) { plan_release(p); return rc; }
    }
    int rc = VSD_OK;
    for (const PlanCall& pc : p->calls) {
      rc = plan_dispatch(ctx, pc.fn, pc.n, pc.a);
      if (rc != VSD_OK) break;
    }
    if (pass == 1) {
      const int rc2 = vsd_graph_end(ctx, (void*)p->stream, &p->graph);
      if (rc == VSD_OK) rc = rc2;
    }
    if (rc != VSD_OK) {
      std::string why = ctx->err;
      plan_release(p);
      return vsd_fail(ctx, rc < 0 && rc > -1000 && why.empty() ? VSD_ERR_ARG : rc, "plan_load: replaying the program failed (%d): %s", rc, why.c_str());
    }
    if (hipStreamSynchronize(p->stream) != hipSuccess) { plan_release(p); return vsd_fail(ctx, VSD_ERR_HIP, "plan_load: the eager pass faulted"); }
  }
  *plan_out = p;
  return VSD_OK;
}

extern "C" int vsd_plan_info(vsd_ctx* ctx, vsd_plan* plan, int* dims) {
  if (!ctx || !plan || !dims) return VSD_ERR_ARG;
  dims[0] = plan->H; dims[1] = plan->W; dims[2] = plan->batch;
  return VSD_OK;
}

extern "C" int vsd_plan_submit(vsd_ctx* ctx, vsd_plan* plan, const void* frame_u8_host, void* out_u8_host) {
  if (!ctx || !plan || !frame_u8_host || !out_u8_host) return VSD_ERR_ARG;
  VSD_HIP(ctx, hipMemcpyAsync(plan->in, frame_u8_host, plan->io_bytes, hipMemcpyHostToDevice, plan->stream));
  VSD_HIP(ctx, hipGraphLaunch((hipGraphExec_t)plan->graph, plan->stream));
  VSD_HIP(ctx, hipMemcpyAsync(out_u8_host, plan->out, plan->io_bytes, hipMemcpyDeviceToHost, plan->stream));
  return VSD_OK;
}

extern "C" int vsd_plan_wait(vsd_ctx* ctx, vsd_plan* plan) {
  if (!ctx || !plan) return VSD_ERR_ARG;
  VSD_HIP(ctx, hipStreamSynchronize(plan->stream));
  return VSD_OK;
}

extern "C" int vsd_plan_infer(vsd_ctx* ctx, vsd_plan* plan, const void* frame_u8_host, void* out_u8_host) {
  const int rc = vsd_plan_submit(ctx, plan, frame_u8_host, out_u8_host);
  return rc != VSD_OK ? rc : vsd_plan_wait(ctx, plan);
}

// A camera frame of any size: crop box (vsd_center_crop_box), upload of the box alone, resample into the plan's input frame, then as
// vsd_plan_submit.  The resample runs in front of the captured graph, not inside it: another source size is another pair of tables.
extern "C" int vsd_plan_submit_frame(vsd_ctx* ctx, vsd_plan* plan, const void* src_u8_host, int src_h, int src_w, int64_t src_row_bytes, void* out_u8_host) {
  if (!ctx || !plan || !src_u8_host || !out_u8_host) return VSD_ERR_ARG;
  if (src_h < 1 || src_w < 1 || src_h > VSD_RESAMPLE_MAX_SIDE || src_w > VSD_RESAMPLE_MAX_SIDE || src_row_bytes < (int64_t)3 * src_w)
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_submit_frame: a %d x %d source with rows of %lld bytes (sides 1..%d, rows of at least 3 * width bytes)", src_w, src_h,
                    (long long)src_row_bytes, VSD_RESAMPLE_MAX_SIDE);
  int box[4];
  if (vsd_center_crop_box(src_w, src_h, plan->W, plan->H, box) != VSD_OK) return vsd_fail(ctx, VSD_ERR_ARG, "plan_submit_frame: no crop box");
  const int bw = box[2] - box[0], bh = box[3] - box[1];
  if (box[0] < 0 || box[1] < 0 || bw < 1 || bh < 1 || box[2] > src_w || box[3] > src_h)
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_submit_frame: the crop box of a %d x %d source for %d x %d is empty", src_w, src_h, plan->W, plan->H);
  const unsigned char* src = (const unsigned char*)src_u8_host + (size_t)box[1] * src_row_bytes + (size_t)box[0] * 3;
  const size_t row = (size_t)bw * 3, one = row * bh, frame = (size_t)plan->H * plan->W * 3;
  if (bw == plan->W && bh == plan->H) {  // already the target size: the box goes straight into the input frame
    for (int b = 0; b < plan->batch; ++b)
      VSD_HIP(ctx, hipMemcpy2DAsync((char*)plan->in + b * frame, row, src + (size_t)b * src_h * src_row_bytes, (size_t)src_row_bytes, row, (size_t)bh,
                                    hipMemcpyHostToDevice, plan->stream));
  } else {
    const char* who = "plan_submit_frame";
    int rc = plan_grow(ctx, plan, who, &plan->raw, &plan->raw_bytes, one * plan->batch);
    if (rc == VSD_OK) rc = plan_grow(ctx, plan, who, &plan->work, &plan->work_bytes, (size_t)vsd_resample_workspace_bytes(bh, plan->W));
    if (rc == VSD_OK) rc = plan_table(ctx, plan, who, &plan->table_x, &plan->table_x_in, bw, plan->W);
    if (rc == VSD_OK) rc = plan_table(ctx, plan, who, &plan->table_y, &plan->table_y_in, bh, plan->H);
    if (rc != VSD_OK) return rc;
    const int whole[4] = {0, 0, bw, bh};
    for (int b = 0; b < plan->batch; ++b) {
      VSD_HIP(ctx, hipMemcpy2DAsync((char*)plan->raw + b * one, row, src + (size_t)b * src_h * src_row_bytes, (size_t)src_row_bytes, row, (size_t)bh,
                                    hipMemcpyHostToDevice, plan->stream));
      rc = vsd_resample_rgb(ctx, (char*)plan->raw + b * one, bh, bw, (int64_t)row, whole, (char*)plan->in + b * frame, plan->H, plan->W, plan->table_x,
                            plan->table_y, plan->work, (void*)plan->stream);
      if (rc != VSD_OK) return rc;
    }
  }
  VSD_HIP(ctx, hipGraphLaunch((hipGraphExec_t)plan->graph, plan->stream));
  VSD_HIP(ctx, hipMemcpyAsync(out_u8_host, plan->out, plan->io_bytes, hipMemcpyDeviceToHost, plan->stream));
  return VSD_OK;
}

extern "C" int vsd_plan_infer_frame(vsd_ctx* ctx, vsd_plan* plan, const void* src_u8_host, int src_h, int src_w, int64_t src_row_bytes, void* out_u8_host) {
  const int rc = vsd_plan_submit_frame(ctx, plan, src_u8_host, src_h, src_w, src_row_bytes, out_u8_host);
  return rc != VSD_OK ? rc : vsd_plan_wait(ctx, plan);
}

// The I420 twin: the camera frame arrives as three planes and the result leaves as packed I420 -- half the bytes both ways.  Only the
// plane rectangles of the crop box travel (widened to an even left / top edge, so that the rectangle starts on a chroma sample and
// the conversion runs in its dword-wide form); the box's odd edge is then the resample's box inside the converted rectangle: the bytes
// of "convert the whole frame, crop, resize".  Conversions and resample are ordinary launches around the captured graph.
extern "C" int vsd_plan_submit_frame_i420(vsd_ctx* ctx, vsd_plan* plan, const void* y_host, int64_t y_stride, const void* u_host, const void* v_host,
                                          int64_t uv_stride, int src_h, int src_w, void* out_i420_host) {
  if (!ctx || !plan || !y_host || !u_host || !v_host || !out_i420_host) return VSD_ERR_ARG;
  const char* who = "plan_submit_frame_i420";
  if (src_h < 1 || src_w < 1 || src_h > VSD_RESAMPLE_MAX_SIDE || src_w > VSD_RESAMPLE_MAX_SIDE || y_stride < src_w || uv_stride < (src_w + 1) / 2)
    return vsd_fail(ctx, VSD_ERR_ARG, "%s: a %d x %d source with rows of %lld / %lld bytes (sides 1..%d, rows of at least width / ceil(width / 2) bytes)", who, src_w,
                    src_h, (long long)y_stride, (long long)uv_stride, VSD_RESAMPLE_MAX_SIDE);
  if ((plan->H | plan->W) & 1) return vsd_fail(ctx, VSD_ERR_ARG, "%s: the plan's %d x %d frame has an odd side: no 4:2:0 output", who, plan->W, plan->H);
  int box[4];
  if (vsd_center_crop_box(src_w, src_h, plan->W, plan->H, box) != VSD_OK) return vsd_fail(ctx, VSD_ERR_ARG, "%s: no crop box", who);
  const int bw = box[2] - box[0], bh = box[3] - box[1];
  if (box[0] < 0 || box[1] < 0 || bw < 1 || bh < 1 || box[2] > src_w || box[3] > src_h)
    return vsd_fail(ctx, VSD_ERR_ARG, "%s: the crop box of a %d x %d source for %d x %d is empty", who, src_w, src_h, plan->W, plan->H);
  const int el = box[0] & ~1, et = box[1] & ~1;            // the uploaded rectangle: even left / top edge
  const int rw = box[2] - el, rh = box[3] - et;            // its luma size
  const int cw = (rw + 1) / 2, ch = (rh + 1) / 2;          // its chroma size
  const size_t ys = ((size_t)rw + 3) & ~(size_t)3, cs = ((size_t)cw + 3) & ~(size_t)3;  // device rows: multiples of 4 bytes
  const size_t one_in = (ys * rh + 2 * cs * ch + 255) & ~(size_t)255;
  const size_t row = ((size_t)rw * 3 + 3) & ~(size_t)3, one_rgb = (row * rh + 255) & ~(size_t)255;
  const size_t frame = (size_t)plan->H * plan->W * 3, frame420 = frame / 2;
  const bool direct = bw == plan->W && bh == plan->H && el == box[0] && et == box[1];  // already the target size: convert into the input frame
  int rc = plan_grow(ctx, plan, who, &plan->yuv_in, &plan->yuv_in_bytes, one_in * plan->batch);
  if (rc == VSD_OK) rc = plan_grow(ctx, plan, who, &plan->yuv_out, &plan->yuv_out_bytes, frame420 * plan->batch);
  if (rc == VSD_OK && !direct) rc = plan_grow(ctx, plan, who, &plan->raw, &plan->raw_bytes, one_rgb * plan->batch);
  if (rc == VSD_OK && !direct) rc = plan_grow(ctx, plan, who, &plan->work, &plan->work_bytes, (size_t)vsd_resample_workspace_bytes(bh, plan->W));
  if (rc == VSD_OK) rc = plan_table(ctx, plan, who, &plan->table_x, &plan->table_x_in, bw, plan->W);
  if (rc == VSD_OK) rc = plan_table(ctx, plan, who, &plan->table_y, &plan->table_y_in, bh, plan->H);
  if (rc != VSD_OK) return rc;
  const int inner[4] = {box[0] - el, box[1] - et, box[0] - el + bw, box[1] - et + bh};
  const size_t src_ch = ((size_t)src_h + 1) / 2;
  for (int b = 0; b < plan->batch; ++b) {
    const unsigned char* hy = (const unsigned char*)y_host + ((size_t)b * src_h + et) * y_stride + el;
    const unsigned char* hu = (const unsigned char*)u_host + ((size_t)b * src_ch + et / 2) * uv_stride + el / 2;
    const unsigned char* hv = (const unsigned char*)v_host + ((size_t)b * src_ch + et / 2) * uv_stride + el / 2;
    unsigned char* dy = (unsigned char*)plan->yuv_in + b * one_in;
    unsigned char *du = dy + ys * rh, *dv = du + cs * ch;
    VSD_HIP(ctx, hipMemcpy2DAsync(dy, ys, hy, (size_t)y_stride, (size_t)rw, (size_t)rh, hipMemcpyHostToDevice, plan->stream));
    VSD_HIP(ctx, hipMemcpy2DAsync(du, cs, hu, (size_t)uv_stride, (size_t)cw, (size_t)ch, hipMemcpyHostToDevice, plan->stream));
    VSD_HIP(ctx, hipMemcpy2DAsync(dv, cs, hv, (size_t)uv_stride, (size_t)cw, (size_t)ch, hipMemcpyHostToDevice, plan->stream));
    if (direct) {
      rc = vsd_i420_to_rgb(ctx, dy, (int64_t)ys, du, dv, (int64_t)cs, 0, 0, rh, rw, (char*)plan->in + b * frame, (int64_t)plan->W * 3, (void*)plan->stream);
    } else {
      rc = vsd_i420_to_rgb(ctx, dy, (int64_t)ys, du, dv, (int64_t)cs, 0, 0, rh, rw, (char*)plan->raw + b * one_rgb, (int64_t)row, (void*)plan->stream);
      if (rc == VSD_OK)
        rc = vsd_resample_rgb(ctx, (char*)plan->raw + b * one_rgb, rh, rw, (int64_t)row, inner, (char*)plan->in + b * frame, plan->H, plan->W, plan->table_x,
                              plan->table_y, plan->work, (void*)plan->stream);
    }
    if (rc != VSD_OK) return rc;
  }
  VSD_HIP(ctx, hipGraphLaunch((hipGraphExec_t)plan->graph, plan->stream));
  const size_t ysz = (size_t)plan->H * plan->W;
  for (int b = 0; b < plan->batch; ++b) {
    unsigned char* o = (unsigned char*)plan->yuv_out + b * frame420;
    rc = vsd_rgb_to_i420(ctx, (char*)plan->out + b * frame, plan->H, plan->W, o, o + ysz, o + ysz + ysz / 4, plan->W, plan->W / 2, (void*)plan->stream);
    if (rc != VSD_OK) return rc;
  }
  VSD_HIP(ctx, hipMemcpyAsync(out_i420_host, plan->yuv_out, frame420 * plan->batch, hipMemcpyDeviceToHost, plan->stream));
  return VSD_OK;
}

extern "C" int vsd_plan_infer_frame_i420(vsd_ctx* ctx, vsd_plan* plan, const void* y_host, int64_t y_stride, const void* u_host, const void* v_host,
                                         int64_t uv_stride, int src_h, int src_w, void* out_i420_host) {
  const int rc = vsd_plan_submit_frame_i420(ctx, plan, y_host, y_stride, u_host, v_host, uv_stride, src_h, src_w, out_i420_host);
  return rc != VSD_OK ? rc : vsd_plan_wait(ctx, plan);
}

// Another prompt for a loaded plan: the bytes of an engine.PromptBlock of the same layout (videosd_amd/plan.py export_prompt) replace
// the plan's -- the C counterpart of VideoSDPipeline's prompt cache (the reference re-encodes the prompt every frame,
// lcm_controlnet.py:115-198; here a prompt is ~40 MB of constants built once).  Waits for the plan's stream first.
extern "C" int vsd_plan_load_prompt(vsd_ctx* ctx, vsd_plan* plan, const char* path) {
  if (!ctx || !plan || !path) return VSD_ERR_ARG;
  FILE* f = fopen(path, "rb");
  if (!f) return vsd_fail(ctx, VSD_ERR_ARG, "plan_load_prompt: cannot open %s", path);
  char magic[8];
  uint64_t n = 0;
  const bool head = fread(magic, 1, 8, f) == 8 && fread(&n, 8, 1, f) == 1 && memcmp(magic, "VSDPRMT1", 8) == 0;
  if (!head || n != plan->prompt_bytes) {
    fclose(f);
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_load_prompt: %s is not a prompt file of this plan's layout (%llu bytes, the plan's block has %zu)", path,
                    (unsigned long long)n, plan->prompt_bytes);
  }
  std::vector<unsigned char> host((size_t)n);
  const bool ok = fread(host.data(), 1, host.size(), f) == host.size();
  fclose(f);
  if (!ok) return vsd_fail(ctx, VSD_ERR_ARG, "plan_load_prompt: %s is truncated", path);
  VSD_HIP(ctx, hipStreamSynchronize(plan->stream));
  VSD_HIP(ctx, hipMemcpy(plan->prompt, host.data(), host.size(), hipMemcpyHostToDevice));
  return VSD_OK;
}

// page-locked host memory for a plan's frames (copies from pageable memory are staged by the runtime and do not overlap other lanes)
extern "C" void* vsd_pinned_alloc(vsd_ctx* ctx, size_t bytes) {
  void* p = nullptr;
  if (!ctx || hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}
extern "C" void vsd_pinned_free(vsd_ctx* ctx, void* p) {
  (void)ctx;
  if (p) (void)hipHostFree(p);
}

extern "C" void vsd_plan_free(vsd_ctx* ctx, vsd_plan* plan) {
  (void)ctx;
  plan_release(plan);
}
