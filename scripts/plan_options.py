"""Live options and shared lanes of a plan file, measured on BASELINE configs[1] (SD1.5 + ControlNet + TAESD, 512x512, 4 steps):
vsd_plan_set_options next to Engine.update_options on the same program, four lanes as four loads against one load + three clones
(time, device memory), the 5 x 4 frame rate of examples/plan_host.c, and what the option tables add to the file.
    python scripts/plan_options.py [--dir /tmp] [--out profiles/plan_options.txt]"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videosd_amd import config as Cf, weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402
from videosd_amd.ops import HipOps  # noqa: E402
from videosd_amd.plan import OPT_ROWS, CPlan, export_plan  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


d = arg("--dir", "/tmp")
out_path = arg("--out", os.path.join(ROOT, "profiles", "plan_options.txt"))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med_ms(ts):
    return 1e3 * float(np.median(ts))


def used_gb():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 1e9


def rate(plans, frame, launches):
    """plan_host's loop through ctypes: frame k goes to lane k mod lanes, pinned buffers, one wait per lane and launch"""
    ctx = plans[0].ctx
    n = frame.nbytes
    bufs = [(ctx.lib.vsd_pinned_alloc(ctx.h, n), ctx.lib.vsd_pinned_alloc(ctx.h, n)) for _ in plans]
    for i, _ in bufs:
        C.memmove(i, frame.ctypes.data, n)
    t = time.perf_counter()
    for k in range(launches):
        l = k % len(plans)
        if k >= len(plans):
            ctx.call("vsd_plan_wait", plans[l].h)
        ctx.call("vsd_plan_submit", plans[l].h, bufs[l][0], bufs[l][1])
    for p in plans:
        ctx.call("vsd_plan_wait", p.h)
    s = time.perf_counter() - t
    for i, o in bufs:
        ctx.lib.vsd_pinned_free(ctx.h, i)
        ctx.lib.vsd_pinned_free(ctx.h, o)
    return launches * plans[0].batch / s


exe = os.path.join(d, "plan_host")
lib = os.path.join(ROOT, "videosd_amd")
subprocess.run(["gcc", "-O2", os.path.join(ROOT, "examples", "plan_host.c"), "-I" + os.path.join(ROOT, "include"), "-L" + lib, "-lvsd", "-Wl,-rpath," + lib,
                "-o", exe], check=True)
ops = HipOps(0)
ops.load_tuning(os.environ.get("VSD_TUNING") or os.path.join(ROOT, "profiles", "tuning_mi355x.json"))
wu = W.synthesize(W.unet_spec(Cf.SD15_UNET), "unet.", device="cuda")
wc = W.synthesize(W.controlnet_spec(Cf.SD15_CONTROLNET), "cn.", device="cuda")
wv = W.synthesize(W.taesd_spec(Cf.TAESD), "vae.", device="cuda")
eng = Engine(ops, Cf.SD15_UNET, Cf.SD15_CONTROLNET, Cf.TAESD, wu, wc, wv)
eng.set_text_embeds((torch.randn(77, 768, generator=torch.Generator().manual_seed(7)) * 0.5).half())
B = 5
eng.tune_for_lanes = True  # (bench.py's rule for coalesced launches on busy lanes)
eng.prepare(512, 512, 4, 0.6, use_controlnet=True, batch=B)
frame = np.random.default_rng(0).integers(0, 256, (B, 512, 512, 3), dtype=np.uint8)
want = eng.infer_u8(frame).copy()
path = os.path.join(d, f"sd15_512_b{B}.vsdplan")
t = time.perf_counter()
info = export_plan(eng, path)
t_exp = time.perf_counter() - t
tables = sum(OPT_ROWS * t_.shape[1] * t_.element_size() for t_ in eng.shared["temb"].values()) + 4 * (OPT_ROWS * 6 + 13)
say(f"plan file, 5 frames per launch: {os.path.getsize(path) / 1e9:.3f} GB, export {t_exp:.1f} s; saved {info['saved_bytes'] / 1e9:.3f} GB of which shareable weights "
    f"{info['shared_bytes'] / 1e9:.3f} GB; option tables (50 rows per network, coefficients, logspace): {tables / 1e6:.2f} MB of the file")

# a slider step: the engine's update_options against the plan's set_options, same program
opts = [(0.3 + 0.02 * (k % 30), 0.05 + 0.1 * (k % 25)) for k in range(40)]
ts = []
for s, c in opts:
    t = time.perf_counter()
    assert eng.update_options(s, c)
    ts.append(time.perf_counter() - t)
say(f"Engine.update_options (returns after its own synchronize): median {med_ms(ts):.3f} ms, min {1e3 * min(ts):.3f}, max {1e3 * max(ts):.3f} over {len(ts)} slider steps")
assert eng.update_options(0.6, 1.0)
base = used_gb()
t = time.perf_counter()
plan = CPlan(path, lane=0)
t_load = time.perf_counter() - t
t_call, t_drain = [], []
for s, c in opts:
    t = time.perf_counter()
    assert plan.set_options(s, c)
    t1 = time.perf_counter()
    plan.ctx.call("vsd_plan_wait", plan.h)
    t_call.append(t1 - t)
    t_drain.append(time.perf_counter() - t)
say(f"vsd_plan_set_options: host call median {med_ms(t_call):.3f} ms (max {1e3 * max(t_call):.3f}); until the stream has drained median {med_ms(t_drain):.3f} ms "
    f"(max {1e3 * max(t_drain):.3f}) over {len(opts)} slider steps")
assert plan.set_options(0.45, 0.8) and eng.update_options(0.45, 0.8)
say(f"after set_options(0.45, 0.8) the plan's frames are the engine's after update_options: {bool(np.array_equal(plan.infer(frame), eng.infer_u8(frame)))}")
assert plan.set_options(0.6, 1.0) and eng.update_options(0.6, 1.0)

# four lanes: one load + three clones against four loads
one = used_gb() - base
t = time.perf_counter()
clones = [plan.clone(lane=l) for l in (1, 2, 3)]
t_clone = time.perf_counter() - t
mem_clones = used_gb() - base
owned, shared = plan.memory()
r_clones = rate([plan] + clones, frame, 120)
same = all(np.array_equal(p.infer(frame), want) for p in [plan] + clones)
for p in clones + [plan]:
    p.close()
del clones, plan
t = time.perf_counter()
loads = [CPlan(path, lane=0)]
loads += [CPlan.__new__(CPlan) for _ in range(3)]
for l in (1, 2, 3):  # (in the first plan's context, as plan_host loaded its lanes before)
    h = C.c_void_p()
    loads[0].ctx.call("vsd_plan_load_lane", path.encode(), l, C.byref(h))
    loads[l].ctx, loads[l].h, loads[l].H, loads[l].W, loads[l].batch = loads[0].ctx, h, loads[0].H, loads[0].W, loads[0].batch
t_loads = time.perf_counter() - t
mem_loads = used_gb() - base
r_loads = rate(loads, frame, 120)
for p in loads:
    p.close()
say(f"one plan: load {t_load:.2f} s, {one:.2f} GB of device memory (vsd_plan_memory: owns {owned / 1e9:.3f} GB, shareable {shared / 1e9:.3f} GB)")
say(f"four lanes as FOUR LOADS: {t_loads:.2f} s, {mem_loads:.2f} GB (hipMemGetInfo), 5 x 4 through ctypes {r_loads:.1f} frames/s")
say(f"four lanes as ONE LOAD + THREE CLONES: {t_load:.2f} + {t_clone:.2f} s, {mem_clones:.2f} GB (hipMemGetInfo; vsd_plan_memory: 4 x {owned / 1e9:.3f} + {shared / 1e9:.3f} "
    f"= {(4 * owned + shared) / 1e9:.2f} GB), 5 x 4 through ctypes {r_clones:.1f} frames/s; every lane bit-identical to the engine: {same}")
open(os.path.join(d, "in.raw"), "wb").write(frame.tobytes())
for extra in ([], ["0.45", "0.8"]):
    r = subprocess.run([exe, path, os.path.join(d, "in.raw"), os.path.join(d, "out.raw"), "120", "4"] + extra, capture_output=True, text=True, timeout=600)
    got = np.frombuffer(open(os.path.join(d, "out.raw"), "rb").read(), dtype=np.uint8).reshape(frame.shape)
    if extra:
        assert eng.update_options(0.45, 0.8)
    say(f"examples/plan_host.c 120 launches on 4 lanes {' '.join(extra) or '(exported options)'}: {r.stdout.strip() or r.stderr.strip()[-300:]}; "
        f"bit-identical to the engine: {bool(np.array_equal(got, eng.infer_u8(frame)))}")
os.remove(path)
open(out_path, "w").write("\n".join(lines) + "\n")
