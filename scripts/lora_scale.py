"""LoRA adapters fused on the device (include/vsd.h THE ADAPTER FUSE; `VideoSDPipeline(loras=[...])`, `set_lora_scale`), measured on BASELINE
configs[1] (SD1.5 + ControlNet + TAESD, 512x512, 4 steps; synthetic weights where no checkpoint is installed; synthetic adapters over
EVERY linear and conv weight of the UNet, written to a temporary directory as kohya-style safetensors files):
  (a) the device time of one vsd_lora_fuse over all adapted tensors at rank 4 / 32 / 128 with one and with four adapters -- between
      events here (`--launches` launches back to back), and from a kernel trace when the leg is run under rocprofv3 and folded in
      (below) -- with the bytes moved (base copies read, packed weights and second copies written, up / down read) over that time, and
      the device memory the base copies and adapters add;
  (b) a whole scale change through the class: `set_lora_scale` (collect, fuse, time tables) and the first frame after it (prompt
      rebuild included), against the only way available before: fuse in torch on the host, build a new Engine, `prepare`, first frame
      -- both timed in the same run;
  (c) the 5 x 4 stream through the class (a worker process, up to 5 frames per launch, 4 launch lanes) with adapters loaded at a fixed
      scale against none, the legs taking turns, `--reps` repetitions each.  The program is the same, so the expectation is "not
      separated by the spread of the repetitions".
Needs a GPU.  `--mini` runs everything on the reduced-width networks at 64 x 64, 2 steps (a check of the script itself, seconds).
    python scripts/lora_scale.py [--reps 3] [--frames 160] [--launches 20] [--out profiles/lora_scale.txt] [--mini]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/lora_scale.py --only-a --launches 5
    python scripts/lora_scale.py --fold-trace DIR [--out profiles/lora_scale.txt]      (appends the kernel times of that trace)"""
import asyncio
import csv
import glob
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videosd_amd import config as C  # noqa: E402
from videosd_amd import weights as W  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


MINI = "--mini" in sys.argv
if MINI:  # (this process and, through the factory below, the worker's)
    C.SD15_UNET, C.SD15_CONTROLNET = C.MINI_UNET, C.MINI_CONTROLNET
reps, n_frames, n_launches = int(arg("--reps", "3")), int(arg("--frames", "160")), int(arg("--launches", "20"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "lora_scale.txt"))
lines = []

BATCH, LANES = 5, 4
OUTSTANDING = (LANES + 1) * BATCH
OPTS = dict(height=64, width=64, strength=0.6, steps=2, controlnet_scale=1.0) if MINI else dict(height=512, width=512, strength=0.6, steps=4, controlnet_scale=1.0)
MODEL = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0)
PROMPT = "a watercolor painting"


def mini_pipeline(**config):
    """factory of the worker process under --mini (`RemotePipeline(factory="lora_scale:mini_pipeline")`)"""
    from videosd_amd.pipeline import VideoSDPipeline

    C.SD15_UNET, C.SD15_CONTROLNET = C.MINI_UNET, C.MINI_CONTROLNET
    return VideoSDPipeline(**config)


def say(s):
    print(s, flush=True)
    lines.append(s)


def write_adapter(directory, spec, rank, seed):
    """a synthetic adapter over every kind-"w" weight of `spec` as a kohya-style safetensors file; alpha = rank / 2"""
    from safetensors.numpy import save_file

    rng = np.random.default_rng(seed)
    out = {}
    for name, shape, kind in spec:
        if kind != "w" or not name.endswith(".weight"):
            continue
        mod = "lora_unet_" + name[:-len(".weight")].replace(".", "_")
        fan_in = int(np.prod(shape[1:]))
        out[f"{mod}.lora_down.weight"] = (rng.standard_normal((rank,) + tuple(shape[1:])) * fan_in ** -0.5).astype(np.float16)
        up = (rng.standard_normal((shape[0], rank)) * 0.02).astype(np.float16)
        out[f"{mod}.lora_up.weight"] = up.reshape(up.shape + (1, 1)) if len(shape) == 4 else up
        out[f"{mod}.alpha"] = np.asarray(rank / 2.0, dtype=np.float32)
    path = os.path.join(directory, f"synthetic_r{rank}_{seed}.safetensors")
    save_file(out, path)
    return path


def unet_weights():
    from videosd_amd import checkpoints as CK
    from videosd_amd.pipeline import load_or_synthesize

    mdir = CK.find_snapshot(MODEL["model"])
    return load_or_synthesize(W.unet_spec(C.SD15_UNET), "unet.", "unet.safetensors", "cpu", CK.checkpoint_file(mdir, "unet"))[0]


# ------------------------------------------------------------------------------------------ (a) the launch
def fuse_cost(tmp, trace_only=False):
    from videosd_amd import lora as LR
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps

    spec = W.unet_spec(C.SD15_UNET)
    wu = unet_weights()
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    eng = Engine(HipOps(0), C.SD15_UNET, C.SD15_CONTROLNET, C.TAESD, wu, None, wv)  # (the UNet alone: the ControlNet is never adapted)
    ops = eng.ops
    if not trace_only:
        say(f"(a) one vsd_lora_fuse over every linear and conv weight of the UNet; {n_launches} launches back to back between two events, "
            "five repetitions; bytes = base copies read + packed weights and second copies written + up / down read")
    for rank in (4, 32, 128):
        paths = [write_adapter(tmp, spec, rank, seed) for seed in range(4)]
        for n in (1, 4):
            ads = [LR.load_adapter(p, spec, name=f"a{i}") for i, p in enumerate(paths[:n])]
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(0)[0]
            aset = eng.load_adapters(ads, wu)
            torch.cuda.synchronize()
            added = free0 - torch.cuda.mem_get_info(0)[0]
            elems = sum(eng.unet.places[t].rows * eng.unet.places[t].pack.k for t in aset.touched)
            copies = sum(eng.unet.places[t].rows * eng.unet.places[t].pack.k for t in aset.touched
                         if eng.unet.places[t].frag or eng.unet.places[t].raw_copy is not None)
            lowrank = sum(a.tensors[t].rank * (eng.unet.places[t].rows + eng.unet.places[t].pack.k) for a in ads for t in a.tensors)
            moved = 2 * (2 * elems + copies + lowrank)
            flop = sum(2 * a.tensors[t].rank * eng.unet.places[t].rows * eng.unet.places[t].pack.k for a in ads for t in a.tensors)
            scales = [0.5 + 0.1 * i for i in range(n)]
            for _ in range(2):
                ops.lora_fuse(aset.table, aset.nseg, scales)
            ops.synchronize()
            ms = []
            for _ in range(1 if trace_only else 5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ops.stream)
                for _i in range(n_launches):
                    ops.lora_fuse(aset.table, aset.nseg, scales)
                e1.record(ops.stream)
                ops.synchronize()
                ms.append(e0.elapsed_time(e1) / n_launches)
            med = float(np.median(ms))
            if not trace_only:
                say(f"  rank {rank}, {n} adapter(s): {aset.nseg} segments, {elems / 1e9:.3f} G elements; {', '.join(f'{v:.3f}' for v in ms)} ms per launch "
                    f"(median {med:.3f} ms); {moved / 1e9:.2f} GB moved: {moved / (med * 1e-3) / 1e9:.0f} GB/s; "
                    f"{flop / 1e9:.1f} GFLOP of fp32 rank steps: {flop / (med * 1e-3) / 1e12:.2f} TFLOP/s; "
                    f"device memory added by base copies, adapters and fold vectors: {added / 2 ** 20:.0f} MiB (base copies alone {aset.base_bytes / 2 ** 20:.0f} MiB)")
            eng.unload_adapters()
            del aset
            torch.cuda.empty_cache()


def fold_trace(directory):
    """the kernel times of a rocprofv3 --kernel-trace of `--only-a`, appended to the profile"""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    us = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "lora_fuse_kernel" in r["Kernel_Name"]:
                us.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = ["(a) by kernel trace (rocprofv3 --kernel-trace of `--only-a`; every launch of lora_fuse_kernel in launch order: rank 4 / 32 / 128, "
           "each with 1 and 4 adapters, warm-up launches included):"]
    out.append("  " + (", ".join(f"{v:.0f}" for v in us) + " us" if us else "(no lora_fuse_kernel in the trace)"))
    for s in out:
        print(s)
    with open(out_path, "a") as fh:
        fh.write("\n".join(out) + "\n")


# ------------------------------------------------------------------------------------------ (b) a whole scale change
def scale_change(tmp):
    from PIL import Image
    from videosd_amd import lora as LR
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps
    from videosd_amd.pipeline import VideoSDPipeline

    spec = W.unet_spec(C.SD15_UNET)
    path = write_adapter(tmp, spec, 32, 100)
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (OPTS["height"], OPTS["width"], 3), dtype=np.uint8), "RGB")
    p = VideoSDPipeline(tuning_mode="table", loras=[{"path": path, "scale": 0.5, "name": "style"}], **MODEL)
    p.infer(img, prompt=PROMPT, **OPTS)
    live = []
    for k in range(max(reps, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.set_lora_scale("style", 0.3 + 0.1 * k)
        t1 = time.perf_counter()
        p.infer(img, prompt=PROMPT, **OPTS)
        live.append((1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))
    say("(b) a whole scale change through the class, one rank-32 adapter over every tensor: set_lora_scale (fuse launch, synchronise) and "
        "the first frame after it (time tables and the cached prompt rebuilt, then the frame):")
    say("  live: " + ", ".join(f"{a:.1f} + {b:.1f} ms" for a, b in live))
    # the only way before: fuse on the host, a new engine, prepare, the first frame
    wu = unet_weights()
    ad = LR.load_adapter(path, spec, name="style")
    wc = W.synthesize(W.controlnet_spec(C.SD15_CONTROLNET), "cn.")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    text = p.encode_prompt(PROMPT)
    frame = np.asarray(img)
    host = []
    for k in range(2):
        t0 = time.perf_counter()
        fused = dict(wu)
        for name, t in ad.tensors.items():
            w = wu[name].float()
            delta = (0.3 + 0.1 * k) * t.a * (t.up.float() @ t.down.float().reshape(t.rank, -1)).reshape(w.shape)
            fused[name] = (w + delta).half()
        t1 = time.perf_counter()
        eng = Engine(HipOps(0), C.SD15_UNET, C.SD15_CONTROLNET, C.TAESD, fused, wc, wv)
        eng.set_text_embeds(text)
        eng.prepare(OPTS["height"], OPTS["width"], OPTS["steps"], OPTS["strength"], controlnet_scale=OPTS["controlnet_scale"], autotune=False)
        t2 = time.perf_counter()
        eng.infer_u8(frame)
        host.append((1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (time.perf_counter() - t2)))
        del eng
    say("  host re-fuse (torch fuse of every tensor + a new Engine with upload and prepare + the first frame): " +
        ", ".join(f"{a:.0f} + {b:.0f} + {c:.0f} ms" for a, b, c in host))
    return path


# ------------------------------------------------------------------------------------------ (c) the 5 x 4 stream
def stream(w, imgs):
    lat = []

    async def go():
        sem = asyncio.Semaphore(OUTSTANDING)

        async def one(fut, t):
            try:
                await fut
                lat.append(time.perf_counter() - t)
            finally:
                sem.release()

        t0 = time.perf_counter()
        tasks = []
        for i in range(n_frames):
            await sem.acquire()
            tasks.append(asyncio.ensure_future(one(w.infer.remote(imgs[i % len(imgs)], prompt=PROMPT, **OPTS), time.perf_counter())))
        await asyncio.gather(*tasks)
        return n_frames / (time.perf_counter() - t0)

    return asyncio.run(go()), 1e3 * float(np.median(lat))


def streams(path):
    from PIL import Image
    from videosd_amd.dispatch import RemotePipeline

    rng = np.random.default_rng(1)
    imgs = [Image.fromarray(rng.integers(0, 256, (OPTS["height"], OPTS["width"], 3), dtype=np.uint8), "RGB") for _ in range(8)]
    extra = dict(factory="lora_scale:mini_pipeline") if MINI else {}
    if MINI:
        os.environ["PYTHONPATH"] = os.path.join(ROOT, "scripts") + os.pathsep + os.environ.get("PYTHONPATH", "")
    workers = {}
    for name, kw in (("no adapters", {}), ("one rank-32 adapter at scale 0.5", dict(loras=[{"path": path, "scale": 0.5, "name": "style"}]))):
        w = RemotePipeline(batch=BATCH, lanes=LANES, shm_slots=OUTSTANDING + 4, call_timeout=600.0, **extra, **MODEL, **kw)
        w.method("warm_up")(batches=tuple(range(1, BATCH + 1)), lanes=LANES, prompt=PROMPT, **OPTS)
        workers[name] = w
    try:
        res = {name: [] for name in workers}
        for name, w in workers.items():
            stream(w, imgs)  # one unrecorded pass
        for _ in range(reps):
            for name, w in workers.items():  # the legs take turns
                res[name].append(stream(w, imgs))
        say(f"(c) 5 x 4 through the class (two worker processes on one GPU taking turns, PIL in / PIL out, {n_frames} frames per repetition, "
            f"{OUTSTANDING} outstanding):")
        for name in workers:
            fps = [r[0] for r in res[name]]
            say(f"  {name}: {', '.join(f'{v:.1f}' for v in fps)} frames/s (median {float(np.median(fps)):.1f}, spread {min(fps):.1f} .. {max(fps):.1f}); "
                f"p50 latency {', '.join(f'{r[1]:.0f}' for r in res[name])} ms")
    finally:
        for w in workers.values():
            w.close()


if __name__ == "__main__":
    if "--fold-trace" in sys.argv:
        fold_trace(arg("--fold-trace", "."))
        sys.exit(0)
    with tempfile.TemporaryDirectory() as tmp:
        if "--only-a" in sys.argv:
            fuse_cost(tmp, trace_only=True)
            sys.exit(0)
        say(f"LoRA adapters fused on the device: {'MINI networks, a check of the script' if MINI else 'SD1.5 + ControlNet + TAESD'}, "
            f"{OPTS['height']} x {OPTS['width']}, {OPTS['steps']} steps; {torch.cuda.get_device_name(0)}")
        fuse_cost(tmp)
        path = scale_change(tmp)
        streams(path)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
