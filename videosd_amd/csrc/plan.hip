// A prepared frame program from a file, for hosts without Python (include/vsd.h vsd_plan_*; format and export: videosd_amd/plan.py).
//
// SURVEY.md section 8b sketched whole-frame C entry points; a frame's sequencing lives in engine.py, so what a non-Python host gets
// is the RECORDED program: every C-ABI call of the engine's one-stream form with its arguments, device pointers as (region, offset).
// vsd_plan_load PARSES the file into a PlanProgram and checks it (argument tags against this library's signatures, interface version
// and signature hash of a format 2 file, every offset against its region) before anything is allocated; then it allocates the regions,
// uploads the saved ones (weights, constants, prompt block, counters), and BINDS: patches the pointers, replays the calls once eagerly
// and once under stream capture, instantiates the graph.  vsd_plan_infer = upload the frame(s), one graph launch, download.  Same
// kernels with the same arguments as the Python engine: the same bits (tests/test_plan_gpu.py).
// vsd_plan_clone_lane binds the same PlanProgram to a second set of regions: the ones flagged as read-only weights are the source's
// (reference-counted), the rest are the clone's own.  vsd_plan_set_options: csrc/plan_options.hip.
#include <stdarg.h>
#include <math.h>
#include <algorithm>
#include <memory>

#include "common.h"
#include "plan_options.h"

namespace {

enum { T_I32 = 0, T_F32 = 1, T_PTR = 2, T_NULL = 3, T_STREAM = 4, T_DESC = 5 };
constexpr int PLAN_MAX_ARGS = 24;
constexpr uint32_t REGION_SHARED = 1;  // region flag, bit 0: read-only network weights, shareable between lanes

union PlanArg {
  void* p;
  int i;
  float f;
};

struct PlanCall {
  int fn, n;
  PlanArg a[PLAN_MAX_ARGS];
};

// per entry point "name:tags" (scripts/gen_plan_dispatch.py): what a recorded call must look like
const char* const PLAN_SIGS[] = {
#define PLAN_DISPATCH_TAGS
#include "plan_dispatch.inc"
#undef PLAN_DISPATCH_TAGS
};
constexpr int PLAN_NFUNCS = (int)(sizeof(PLAN_SIGS) / sizeof(PLAN_SIGS[0]));

const char* plan_tags(int fn) { return strchr(PLAN_SIGS[fn], ':') + 1; }

bool plan_fn_is(int fn, const char* name) {
  const size_t n = strlen(name);
  return strncmp(PLAN_SIGS[fn], name, n) == 0 && PLAN_SIGS[fn][n] == ':';
}

uint64_t plan_signature_hash() {  // FNV-1a over the lines, each followed by a newline (videosd_amd/plan.py signature_hash)
  uint64_t h = 0xCBF29CE484222325ull;
  for (int i = 0; i < PLAN_NFUNCS; ++i)
    for (const char* c = PLAN_SIGS[i];; ++c) {
      h = (h ^ (unsigned char)(*c ? *c : '\n')) * 0x100000001B3ull;
      if (!*c) break;
    }
  return h;
}

// ---- the file as parsed: what every plan of this program shares on the host
struct RawArg {
  uint32_t tag, aux;  // (T_DESC: aux = index into `blobs`)
  uint64_t val;
};
struct RawCall {
  int fn, n;
  RawArg a[PLAN_MAX_ARGS];
};
struct RawFix {
  uint32_t boff, reg;
  uint64_t off;
};
struct RawBlob {
  std::vector<unsigned char> bytes;
  std::vector<RawFix> fix;
};
struct RawOptTable {
  uint32_t table_r, live_r;
  uint64_t table_off, live_off, live_stride, row_bytes;
};
struct PlanProgram {
  uint32_t version = 0;
  int H = 0, W = 0, batch = 0;
  std::vector<uint64_t> size;
  std::vector<uint32_t> saved, flags;
  uint32_t in_r = 0, out_r = 0, pr_r = 0;
  uint64_t in_off = 0, out_off = 0, pr_off = 0, pr_bytes = 0;
  std::vector<RawCall> calls;
  std::vector<RawBlob> blobs;
  // the options section (format 2)
  bool options = false;
  uint32_t n = 0, steps = 0, nres = 0;
  uint32_t consts_r = 0, coef_r = 0;
  uint64_t consts_off = 0, coef_off = 0;
  std::vector<RawOptTable> tabs;
  // per-frame seeds: where the program's vsd_add_noise_seeded calls read them (no field of the file: found in the call list)
  bool seeded = false;
  uint32_t seed_r = 0;
  uint64_t seed_off = 0;
};

}  // namespace

struct vsd_plan {
  vsd_ctx* ctx = nullptr;
  int H = 0, W = 0, batch = 0;
  std::shared_ptr<const PlanProgram> prog;
  std::vector<std::shared_ptr<void>> regions;     // (a region flagged REGION_SHARED may belong to several plans: freed with the last)
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

// vsd_plan_set_seeds: up to 32 seeds per launch, by value
struct SeedChunk {
  uint64_t v[32];
};
__global__ void plan_set_seeds_kernel(uint64_t* __restrict__ dst, SeedChunk c, int n) {
  const int i = threadIdx.x;
  if (i < n) dst[i] = c.v[i];
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
  p->regions.clear();
  for (void* r : {p->raw, p->work, p->table_x, p->table_y, p->yuv_in, p->yuv_out})
    if (r) (void)hipFree(r);
  delete p;
}

std::shared_ptr<void> region_alloc(uint64_t bytes) {
  void* d = nullptr;
  if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess) return nullptr;
  return std::shared_ptr<void>(d, [](void* q) { (void)hipFree(q); });
}

// [off, off + bytes) inside region `reg`
bool plan_inside(const PlanProgram& g, uint32_t reg, uint64_t off, uint64_t bytes) {
  return reg < g.size.size() && off <= g.size[reg] && bytes <= g.size[reg] - off;
}

// Parse and check a plan file up to the bytes of its regions (`f` is left there).  Nothing here touches the device.
const char* plan_parse(FILE* f, PlanProgram& g) {
  Reader r{f};
  g.version = r.get<uint32_t>();
  g.H = (int)r.get<uint32_t>();
  g.W = (int)r.get<uint32_t>();
  g.batch = (int)r.get<uint32_t>();
  const uint32_t nreg = r.get<uint32_t>(), ncall = r.get<uint32_t>();
  g.in_r = r.get<uint32_t>();
  g.in_off = r.get<uint64_t>();
  g.out_r = r.get<uint32_t>();
  g.out_off = r.get<uint64_t>();
  g.pr_r = r.get<uint32_t>();
  g.pr_off = r.get<uint64_t>();
  g.pr_bytes = r.get<uint64_t>();
  if (!r.ok || (g.version != 1 && g.version != 2) || nreg == 0 || nreg > (1u << 20) || ncall == 0 || ncall > (1u << 22) || g.in_r >= nreg || g.out_r >= nreg ||
      g.H < 1 || g.W < 1 || g.batch < 1 || g.H > (1 << 16) || g.W > (1 << 16) || g.batch > (1 << 10))
    return "bad header";
  uint32_t ntab = 0;
  if (g.version >= 2) {
    const uint32_t ext = r.get<uint32_t>(), iface = r.get<uint32_t>();
    const uint64_t hash = r.get<uint64_t>();
    if (!r.ok) return "truncated extension";
    if (iface != VSD_VERSION) return "written for another interface version of the library: export the plan again";
    if (hash != plan_signature_hash()) return "written against other entry point signatures: export the plan again";
    g.n = r.get<uint32_t>();
    g.steps = r.get<uint32_t>();
    g.nres = r.get<uint32_t>();
    ntab = r.get<uint32_t>();
    (void)r.get<double>();  // strength and ControlNet scale as exported: the live constants hold them already
    (void)r.get<double>();
    g.consts_r = r.get<uint32_t>();
    g.coef_r = r.get<uint32_t>();
    g.consts_off = r.get<uint64_t>();
    g.coef_off = r.get<uint64_t>();
    if (!r.ok) return "truncated options section";
    if (g.n < 1 || g.n > (uint32_t)PLAN_OPT_ROWS || g.steps < g.n || g.steps > 1000 || g.nres < 1 || g.nres > 64 || ntab < 1 || ntab > (uint32_t)PLAN_OPT_TABLES || ext != 12 + 56 + 40 * ntab)
      return "bad options section";
    g.tabs.resize(ntab);
    for (RawOptTable& t : g.tabs) {
      t.table_r = r.get<uint32_t>();
      t.live_r = r.get<uint32_t>();
      t.table_off = r.get<uint64_t>();
      t.live_off = r.get<uint64_t>();
      t.live_stride = r.get<uint64_t>();
      t.row_bytes = r.get<uint64_t>();
    }
    if (!r.ok) return "truncated options section";
    g.options = true;
  }
  g.size.resize(nreg);
  g.saved.resize(nreg);
  g.flags.resize(nreg);
  for (uint32_t i = 0; i < nreg; ++i) {
    g.size[i] = r.get<uint64_t>();
    g.saved[i] = r.get<uint32_t>();
    g.flags[i] = g.version >= 2 ? r.get<uint32_t>() : ((void)r.get<uint32_t>(), 0u);
    if (r.ok && (g.size[i] > (1ull << 40) || ((g.flags[i] & REGION_SHARED) && !g.saved[i]))) return "bad region table";
  }
  if (!r.ok) return "truncated region table";
  if (g.options) {
    // what vsd_plan_set_options reads and writes, checked once: inside saved regions, dword-aligned, and never in a shared region
    auto rw = [&](uint32_t reg, uint64_t off, uint64_t bytes, bool written) {
      return plan_inside(g, reg, off, bytes) && off % 4 == 0 && g.saved[reg] && !(written && (g.flags[reg] & REGION_SHARED));
    };
    if (!rw(g.consts_r, g.consts_off, 4ull * (2 + PLAN_OPT_COEF * g.n + g.nres), true) ||
        !rw(g.coef_r, g.coef_off, 4ull * (PLAN_OPT_ROWS * PLAN_OPT_COEF + g.nres), false))
      return "option constants outside their regions";
    for (const RawOptTable& t : g.tabs)
      if (t.row_bytes == 0 || t.row_bytes % 4 || t.live_stride % 4 || t.live_stride < t.row_bytes || t.row_bytes > (1ull << 30) || t.live_stride > (1ull << 30) ||
          !rw(t.table_r, t.table_off, t.row_bytes * PLAN_OPT_ROWS, false) || !rw(t.live_r, t.live_off, t.live_stride * (g.n - 1) + t.row_bytes, true))
        return "option tables outside their regions";
  }
  g.calls.resize(ncall);
  for (uint32_t c = 0; c < ncall; ++c) {
    RawCall& rc = g.calls[c];
    rc.fn = (int)r.get<uint32_t>();
    rc.n = (int)r.get<uint32_t>();
    if (!r.ok || rc.fn < 0 || rc.fn >= PLAN_NFUNCS || rc.n < 0 || rc.n > PLAN_MAX_ARGS) return "bad call record";
    const char* tags = plan_tags(rc.fn);
    if ((size_t)rc.n != strlen(tags)) return "a call with another number of arguments than its entry point takes";
    int desc_count = -1, desc_at = -1;
    for (int k = 0; k < rc.n; ++k) {
      RawArg& a = rc.a[k];
      a.tag = r.get<uint32_t>();
      a.aux = r.get<uint32_t>();
      a.val = r.get<uint64_t>();
      if (!r.ok) return "truncated call list";
      // the tag against the entry point's signature: an integer where a pointer is expected never reaches the call
      bool fits = false;
      switch (tags[k]) {
        case 'i': fits = a.tag == T_I32; break;
        case 'f': fits = a.tag == T_F32; break;
        case 'p': fits = a.tag == T_PTR || a.tag == T_STREAM || a.tag == T_NULL; break;  // (a pointer may be optional: the entry point says)
        case 'd': fits = a.tag == T_DESC; break;
        case 'o': fits = a.tag == T_NULL; break;
      }
      if (a.tag > T_DESC) return "unknown argument tag";
      if (!fits) return "an argument tag that does not fit its entry point's signature";
      if (a.tag == T_PTR && !plan_inside(g, a.aux, a.val, 1)) return "pointer outside its region";
      if (a.tag == T_DESC) {
        if (a.aux == 0 || a.aux > VSD_CONV_GROUP_MAX || a.val != (uint64_t)a.aux * sizeof(vsd_conv_desc)) return "descriptor array of another interface version";
        RawBlob blob;
        blob.bytes.resize((size_t)a.val);
        r.bytes(blob.bytes.data(), blob.bytes.size());
        const uint32_t nfix = r.get<uint32_t>();
        if (!r.ok || nfix > 64 * a.aux) return "bad descriptor record";
        blob.fix.resize(nfix);
        for (RawFix& x : blob.fix) {
          x.boff = r.get<uint32_t>();
          x.reg = r.get<uint32_t>();
          x.off = r.get<uint64_t>();
          if (!r.ok || (uint64_t)x.boff + sizeof(void*) > blob.bytes.size() || !plan_inside(g, x.reg, x.off, 1)) return "bad descriptor pointer";
        }
        desc_count = (int)a.aux;
        desc_at = k;
        a.aux = (uint32_t)g.blobs.size();
        g.blobs.push_back(std::move(blob));
      }
    }
    // a descriptor array is followed by its count (vsd_conv_gemm_group) or is one descriptor (vsd_conv_gemm)
    if (desc_at >= 0) {
      const bool counted = desc_at + 1 < rc.n && tags[desc_at + 1] == 'i';
      if (counted ? (int)(int64_t)rc.a[desc_at + 1].val != desc_count : desc_count != 1) return "a descriptor array of another length than its call says";
    }
    // the seed buffer of a program with seeded noise: `seeds_dev` (argument 1) of its vsd_add_noise_seeded calls -- ONE buffer of 8 bytes
    // per frame of the launch, in a saved region of the plan's own
    if (plan_fn_is(rc.fn, "vsd_add_noise_seeded")) {
      const RawArg& a = rc.a[1];
      if (a.tag != T_PTR || a.val % 8 || !plan_inside(g, a.aux, a.val, 8ull * g.batch) || !g.saved[a.aux] || (g.flags[a.aux] & REGION_SHARED))
        return "the seeds of a seeded noise call outside a region of the plan's own";
      if (g.seeded && (g.seed_r != a.aux || g.seed_off != a.val)) return "seeded noise calls with different seed buffers";
      g.seeded = true;
      g.seed_r = a.aux;
      g.seed_off = a.val;
    }
  }
  if (!plan_inside(g, g.in_r, g.in_off, (uint64_t)g.batch * g.H * g.W * 3) || !plan_inside(g, g.out_r, g.out_off, (uint64_t)g.batch * g.H * g.W * 3) ||
      !plan_inside(g, g.pr_r, g.pr_off, g.pr_bytes) || g.in_off >= g.size[g.in_r] || g.out_off >= g.size[g.out_r] || g.pr_off >= g.size[g.pr_r])
    return "frame buffers / prompt block outside their regions";
  return nullptr;
}

// The plan's regions are in place: patch the program's pointers into this plan's calls and descriptor arrays, then one eager pass
// (first-touch of every kernel, the error reports of the ops) and the captured one.  On failure the caller releases the plan.
int plan_bind(vsd_ctx* ctx, vsd_plan* p, const char* who) {
  const PlanProgram& g = *p->prog;
  auto at = [&](uint32_t reg, uint64_t off) { return (void*)((char*)p->regions[reg].get() + off); };
  p->H = g.H; p->W = g.W; p->batch = g.batch;
  p->blobs.resize(g.blobs.size());
  for (size_t b = 0; b < g.blobs.size(); ++b) {
    p->blobs[b] = g.blobs[b].bytes;
    for (const RawFix& x : g.blobs[b].fix) {
      void* q = at(x.reg, x.off);
      memcpy(p->blobs[b].data() + x.boff, &q, sizeof(void*));
    }
  }
  p->calls.resize(g.calls.size());
  for (size_t c = 0; c < g.calls.size(); ++c) {
    const RawCall& rc = g.calls[c];
    PlanCall& pc = p->calls[c];
    pc.fn = rc.fn;
    pc.n = rc.n;
    for (int k = 0; k < rc.n; ++k) {
      const RawArg& a = rc.a[k];
      pc.a[k].p = nullptr;
      switch (a.tag) {
        case T_I32: pc.a[k].i = (int)(int64_t)a.val; break;
        case T_F32: { const uint32_t b = (uint32_t)a.val; memcpy(&pc.a[k].f, &b, 4); break; }
        case T_PTR: pc.a[k].p = at(a.aux, a.val); break;
        case T_STREAM: pc.a[k].p = (void*)p->stream; break;
        case T_DESC: pc.a[k].p = p->blobs[a.aux].data(); break;
        default: break;
      }
    }
  }
  p->in = at(g.in_r, g.in_off);
  p->out = at(g.out_r, g.out_off);
  p->prompt = at(g.pr_r, g.pr_off);
  p->prompt_bytes = (size_t)g.pr_bytes;
  p->io_bytes = (size_t)p->batch * p->H * p->W * 3;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      int rc = vsd_graph_begin(ctx, (void*)p->stream);
      if (rc != VSD_OK) return rc;
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
      return vsd_fail(ctx, rc < 0 && rc > -1000 && why.empty() ? VSD_ERR_ARG : rc, "%s: replaying the program failed (%d): %s", who, rc, why.c_str());
    }
    if (hipStreamSynchronize(p->stream) != hipSuccess) return vsd_fail(ctx, VSD_ERR_HIP, "%s: the eager pass faulted", who);
  }
  return VSD_OK;
}

// the plan's launch stream: lane >= 0: launch stream `lane` of the process's pool, else one of the plan's own
bool plan_stream(vsd_ctx* ctx, vsd_plan* p, int lane) {
  if (lane >= 0) {
    void* pool[VSD_POOL_STREAMS];
    if (vsd_stream_pool(ctx, pool) != VSD_OK) return false;
    p->stream = (hipStream_t)pool[lane];
    p->own_stream = false;
    return true;
  }
  return hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) == hipSuccess;
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
  char magic[8];
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "VSDPLAN1", 8) != 0) {
    fclose(f);
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_load: %s is not a plan file", path);
  }
  vsd_plan* p = nullptr;
  auto fail = [&](const char* what) {
    fclose(f);
    plan_release(p);
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_load: %s (%s)", what, path);
  };
  auto prog = std::make_shared<PlanProgram>();
  if (const char* why = plan_parse(f, *prog)) return fail(why);
  // the bytes of the saved regions must all be there before the first allocation: a cut file costs nothing
  {
    uint64_t need = 0;
    for (size_t i = 0; i < prog->size.size(); ++i)
      if (prog->saved[i]) need += prog->size[i];
    const long here = ftell(f);
    if (here < 0 || fseek(f, 0, SEEK_END) != 0) return fail("cannot seek");
    const long total = ftell(f);
    if (total < 0 || (uint64_t)(total - here) < need) return fail("truncated region contents");
    if (fseek(f, here, SEEK_SET) != 0) return fail("cannot seek");
  }
  const PlanProgram& g = *prog;
  const size_t nreg = g.size.size();
  p = new vsd_plan;
  p->ctx = ctx;
  p->prog = prog;
  (void)hipSetDevice(ctx->device);
  if (!plan_stream(ctx, p, lane)) return fail("no launch stream");
  p->regions.assign(nreg, nullptr);
  for (size_t i = 0; i < nreg; ++i) {
    if (!(p->regions[i] = region_alloc(g.size[i]))) return fail("out of device memory");
    if (!g.saved[i] && hipMemsetAsync(p->regions[i].get(), 0, g.size[i], p->stream) != hipSuccess) return fail("hipMemset failed");
  }
  {
    std::vector<unsigned char> host(1 << 24);
    for (size_t i = 0; i < nreg; ++i) {
      if (!g.saved[i]) continue;
      uint64_t done = 0;
      while (done < g.size[i]) {
        const size_t n = (size_t)std::min<uint64_t>(host.size(), g.size[i] - done);
        if (fread(host.data(), 1, n, f) != n) return fail("truncated region contents");
        if (hipMemcpy((char*)p->regions[i].get() + done, host.data(), n, hipMemcpyHostToDevice) != hipSuccess) return fail("upload failed");
        done += n;
      }
    }
  }
  fclose(f);
  f = nullptr;
  const int rc = plan_bind(ctx, p, "plan_load");
  if (rc != VSD_OK) {
    plan_release(p);
    return rc;
  }
  *plan_out = p;
  return VSD_OK;
}

// A second plan of the same program that shares the source's read-only weights (include/vsd.h).
extern "C" int vsd_plan_clone_lane(vsd_ctx* ctx, vsd_plan* src, int lane, vsd_plan** plan_out) {
  if (!ctx || !src || !plan_out) return VSD_ERR_ARG;
  if (lane >= VSD_POOL_STREAMS) return vsd_fail(ctx, VSD_ERR_ARG, "plan_clone_lane: lane %d (0..%d, or -1 for a stream of the plan's own)", lane, VSD_POOL_STREAMS - 1);
  *plan_out = nullptr;
  (void)hipSetDevice(ctx->device);
  VSD_HIP(ctx, hipStreamSynchronize(src->stream));  // what the clone copies is what the source's last frame left
  const PlanProgram& g = *src->prog;
  vsd_plan* p = new vsd_plan;
  p->ctx = ctx;
  p->prog = src->prog;
  auto fail = [&](int code, const char* what) {
    plan_release(p);
    return vsd_fail(ctx, code, "plan_clone_lane: %s", what);
  };
  if (!plan_stream(ctx, p, lane)) return fail(VSD_ERR_HIP, "no launch stream");
  const size_t nreg = g.size.size();
  p->regions.assign(nreg, nullptr);
  for (size_t i = 0; i < nreg; ++i) {
    if (g.flags[i] & REGION_SHARED) {
      p->regions[i] = src->regions[i];
      continue;
    }
    if (!(p->regions[i] = region_alloc(g.size[i]))) return fail(VSD_ERR_NOMEM, "out of device memory");
    const hipError_t e = g.saved[i] ? hipMemcpyAsync(p->regions[i].get(), src->regions[i].get(), g.size[i], hipMemcpyDeviceToDevice, p->stream)
                                    : hipMemsetAsync(p->regions[i].get(), 0, g.size[i], p->stream);
    if (e != hipSuccess) return fail(VSD_ERR_HIP, "copying the source's regions failed");
  }
  const int rc = plan_bind(ctx, p, "plan_clone_lane");
  if (rc != VSD_OK) {
    plan_release(p);
    return rc;
  }
  *plan_out = p;
  return VSD_OK;
}

extern "C" int vsd_plan_memory(vsd_ctx* ctx, vsd_plan* plan, uint64_t* out) {
  if (!ctx || !plan || !out) return VSD_ERR_ARG;
  const PlanProgram& g = *plan->prog;
  out[0] = out[1] = 0;
  for (size_t i = 0; i < g.size.size(); ++i) out[(g.flags[i] & REGION_SHARED) ? 1 : 0] += g.size[i];
  return VSD_OK;
}

// lcm.lcm_timesteps (videosd_amd/lcm.py) on the host, in the same double arithmetic: 50 * strength truncated towards zero
extern "C" int vsd_lcm_timesteps(double strength, int steps, int* out, int* n) {
  if (!out || !n) return VSD_ERR_ARG;
  *n = 0;
  if (steps < 1 || !(strength == strength) || strength > 1e6 || strength < -1e6) return VSD_ERR_ARG;
  const int origin = (int)(50.0 * strength);  // origin timesteps 19, 39, ...: index j holds 20 (j + 1) - 1
  if (origin < 1) return VSD_ERR_ARG;         // an empty schedule
  const int skipping = std::max(origin / steps, 1);
  int count = 0;
  for (int j = origin - 1; j >= 0 && count < steps; j -= skipping) out[count++] = 20 * (j + 1) - 1;
  *n = count;
  return VSD_OK;
}

// Engine.update_options for a loaded plan: include/vsd.h; the launch: csrc/plan_options.hip
extern "C" int vsd_plan_set_options(vsd_ctx* ctx, vsd_plan* plan, double strength, double controlnet_scale) {
  if (!ctx || !plan) return VSD_ERR_ARG;
  const PlanProgram& g = *plan->prog;
  if (!g.options)
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_set_options: the plan file has format version %u, which holds no option tables: export the plan again", g.version);
  std::vector<int> ts(g.steps);
  int n = 0;
  if (vsd_lcm_timesteps(strength, (int)g.steps, ts.data(), &n) != VSD_OK)
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_set_options: strength %g gives an empty LCM schedule", strength);
  if (n != (int)g.n) return VSD_PLAN_OTHER_PROGRAM;
  PlanOptArgs a{};
  for (int i = 0; i < n; ++i) {
    const int row = (ts[i] + 1) / 20 - 1;
    if ((ts[i] + 1) % 20 != 0 || row < 0 || row >= PLAN_OPT_ROWS) return VSD_PLAN_OTHER_PROGRAM;
    a.row[i] = (unsigned char)row;
  }
  auto at = [&](uint32_t reg, uint64_t off) { return (void*)((char*)plan->regions[reg].get() + off); };
  a.n = n;
  a.nres = (int)g.nres;
  a.ntab = (int)g.tabs.size();
  a.scale = (float)controlnet_scale;
  a.coef = (const float*)at(g.coef_r, g.coef_off);
  a.consts = (float*)at(g.consts_r, g.consts_off);
  for (int t = 0; t < a.ntab; ++t) {
    const RawOptTable& r = g.tabs[t];
    a.tab[t] = {(const uint32_t*)at(r.table_r, r.table_off), (uint32_t*)at(r.live_r, r.live_off), (uint32_t)(r.row_bytes / 4), (uint32_t)(r.live_stride / 4)};
  }
  return plan_options_launch(ctx, plan->stream, a);
}

// one seed per frame of the launch for the frames submitted from now on: include/vsd.h
extern "C" int vsd_plan_set_seeds(vsd_ctx* ctx, vsd_plan* plan, const uint64_t* seeds, int n) {
  if (!ctx || !plan) return VSD_ERR_ARG;
  const PlanProgram& g = *plan->prog;
  if (!g.seeded)
    return vsd_fail(ctx, VSD_ERR_ARG, "plan_set_seeds: the plan's program holds no seeded noise (export it from an engine prepared with device_seed)");
  if (!seeds || n != plan->batch) return vsd_fail(ctx, VSD_ERR_ARG, "plan_set_seeds: %d seed(s) given, the plan takes %d frame(s) per launch", seeds ? n : 0, plan->batch);
  // The values travel as kernel ARGUMENTS, 32 per launch: read when the call is made (the caller's array is free at once, pinned or
  // not), written in stream order, and no copy from pageable memory that would wait for the frames in flight on this stream.
  // (a u64 in memory is the (low, high) u32 pair the noise kernels read: little-endian, as the plan file itself)
  uint64_t* dst = (uint64_t*)((char*)plan->regions[g.seed_r].get() + g.seed_off);
  for (int at = 0; at < n; at += 32) {
    SeedChunk c{};
    const int m = std::min(32, n - at);
    for (int i = 0; i < m; ++i) c.v[i] = seeds[at + i];
    LaunchScope ls(ctx, plan->stream, VSD_FAM_ELEMENTWISE, 0.0);
    hipLaunchKernelGGL(plan_set_seeds_kernel, dim3(1), dim3(64), 0, plan->stream, dst + at, c, m);
    const int rc = ls.finish();
    if (rc != VSD_OK) return rc;
  }
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
