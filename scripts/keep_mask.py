"""What the keep-mask stages (VideoSDPipeline(keep_mask=True); include/vsd.h THE KEEP MASK; csrc/keep_mask.hip, vsd_latent_keep in
csrc/noise.hip) cost, in ONE run.  Writes profiles/keep_mask.txt.
  (1) the three kernels at five 512 x 512 frames per call, per call between device events (calls back to back on one stream: the kernel
      and the gap behind it), in a child process of this script: `mask_blend` with an all-255, an all-0 and a half mask, `mask_latent`,
      `latent_keep` in its step form (table noise and seeds) and its final form, next to the bytes a call must move.
  (2) the stream: BASELINE.json configs[1] (512 x 512, 4 steps, ControlNet) through the drop-in class at the bench's operating point --
      worker mode, up to 5 frames per launch, 4 launch lanes -- with the switch off, on with all-255 masks (no `set_mask`), and on with a
      half mask, repetitions taking turns.  The off leg records the default programs; the on legs are reported against it, with the
      spread between the off repetitions as the noise floor.
Run on the GPU box:
    python scripts/keep_mask.py [--reps 3] [--frames 160] [--swap] [--out profiles/keep_mask.txt]
    python scripts/keep_mask.py --op            (what the child runs: 200 calls per case, back to back on one stream)"""
import asyncio
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps, n_frames = int(arg("--reps", "3")), int(arg("--frames", "160"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "keep_mask.txt"))
lines = []

BATCH, LANES = 5, 4
OPTS = dict(height=512, width=512, steps=4, prompt="pixar, cg", strength=0.6, controlnet_scale=1.0)
MODEL = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0)
H = W = 512
OP_CALLS = 200


def say(s):
    print(s, flush=True)
    lines.append(s)


def half_mask(h, w):
    m = np.full((h, w), 255, np.uint8)
    m[:, :w // 2] = 0
    return m


def op_loop():
    """per case OP_CALLS calls back to back; prints the time per call between device events"""
    import torch

    from videosd_amd.ops import HipOps

    ops = HipOps(0)
    dev = ops.device
    rng = np.random.default_rng(0)
    hw = (H // 8) * (W // 8)
    src = torch.from_numpy(rng.integers(0, 256, (BATCH, H, W, 3), dtype=np.uint8)).to(dev)
    dst = torch.from_numpy(rng.integers(0, 256, (BATCH, H, W, 3), dtype=np.uint8)).to(dev)
    masks = {"all 255": np.full((BATCH, H, W), 255, np.uint8), "all 0": np.zeros((BATCH, H, W), np.uint8),
             "half": np.broadcast_to(half_mask(H, W), (BATCH, H, W)).copy()}
    masks = {k: torch.from_numpy(v).to(dev) for k, v in masks.items()}
    wl = torch.zeros(BATCH, hw, dtype=torch.float32, device=dev)
    x0, lat, den, dec = (torch.randn(BATCH * hw, 8, device=dev).half() for _ in range(4))
    table = torch.randn(4, hw, dtype=torch.float32, device=dev)
    seeds = torch.arange(BATCH, dtype=torch.int64, device=dev)
    coef = torch.tensor([0.9, 0.4, 0.1, 0.9, 0.95, 0.3], dtype=torch.float32, device=dev)
    rgb_mb, lat_mb = BATCH * H * W * 3 / 1e6, BATCH * hw * 16 / 1e6
    cases = [(f"mask_blend, {k} masks", lambda m=m: ops.mask_blend(src, dst, m, BATCH, H, W), f"{3 * rgb_mb + rgb_mb / 3:.2f} MB") for k, m in masks.items()]
    cases.append(("mask_latent", lambda: ops.mask_latent(masks["half"], BATCH, H, W, wl), f"{rgb_mb / 3:.2f} MB"))
    cases.append(("latent_keep, step form, table noise", lambda: ops.latent_keep(x0, wl, table, None, 0, 0, coef, 0, hw, BATCH, lat=lat), f"{3 * lat_mb:.2f} MB"))
    cases.append(("latent_keep, step form, seeds", lambda: ops.latent_keep(x0, wl, None, seeds, 0, 0, coef, 0, hw, BATCH, lat=lat), f"{3 * lat_mb:.2f} MB"))
    cases.append(("latent_keep, final form", lambda: ops.latent_keep(x0, wl, None, None, 0, 0, None, 0, hw, BATCH, den=den, dec_in=dec), f"{4 * lat_mb:.2f} MB"))
    torch.cuda.synchronize()
    ops.mask_latent(masks["half"], BATCH, H, W, wl)  # (the weights of the half mask: half the latent rows take the early exit, half do not)
    for name, call, mb in cases:
        for _ in range(20):  # warm-up: code objects
            call()
        ops.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ops.stream)
        for _ in range(OP_CALLS):
            call()
        e1.record(ops.stream)
        ops.synchronize()
        print(f"op {name}: {e0.elapsed_time(e1) * 1e3 / OP_CALLS:.1f} us per call between events ({mb} to move)", flush=True)


def kernel_times():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--op"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:  # (possibly a fault on the card: nothing more is started on it)
        raise SystemExit(f"(1) the op loop failed (exit {r.returncode}): {r.stderr[-400:]}")
    say(f"(1) per call between device events, five {W} x {H} frames per call ({OP_CALLS} calls back to back on one stream: the kernel and the gap behind it):")
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("op "):
            say("  " + ln[3:])
            got[ln[3:].split(":")[0]] = float(ln.split(": ")[1].split(" us")[0])
    return got


def worker(keep, mask):
    from videosd_amd.pipeline import VideoSDPipeline

    kw = dict(keep_mask=True) if keep else {}
    w = VideoSDPipeline.remote(batch=BATCH, lanes=LANES, shm_slots=(LANES + 1) * BATCH + 4, call_timeout=600.0, **kw, **MODEL)
    if mask is not None:
        w.method("set_mask")(mask)
    w.method("warm_up")(batches=tuple(range(1, BATCH + 1)), lanes=LANES, **OPTS)
    return w


def stream(w, imgs):
    """`n_frames` frames, (LANES + 1) * BATCH outstanding -> (frames/s, frames per launch)"""
    before = w.metrics()

    async def go():
        sem = asyncio.Semaphore((LANES + 1) * BATCH)

        async def one(i):
            async with sem:
                await w.infer.remote(imgs[i % len(imgs)], **OPTS)

        t0 = time.perf_counter()
        await asyncio.gather(*[one(i) for i in range(n_frames)])
        return n_frames / (time.perf_counter() - t0)

    fps = asyncio.run(go())
    after = w.metrics()
    return fps, (after["frames"] - before["frames"]) / max(after["launches"] - before["launches"], 1)


def frame_rates(ops_us):
    from PIL import Image

    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:512, 0:512]
    imgs = [Image.fromarray((rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) // 2 + ((xx * 2 + yy + 17 * i) % 256).astype(np.uint8)[..., None] // 2), "RGB")
            for i in range(8)]  # (bench.py's synthetic frames: seeded noise blended with a moving gradient)
    legs = {"off": (False, None), "on, all 255": (True, None), "on, half mask": (True, half_mask(360, 640))}  # (a mask of another size: sized once per plan size)
    if "--swap" in sys.argv:  # the two on-legs' workers made, and run, in the other order: is a difference between them the leg's or the process's?
        legs = {k: legs[k] for k in ("off", "on, half mask", "on, all 255")}
    workers = {}
    try:
        for name, (keep, mask) in legs.items():
            t0 = time.perf_counter()
            workers[name] = worker(keep, mask)
            print(f"worker keep_mask {name}: loaded and warmed in {time.perf_counter() - t0:.0f} s", flush=True)
        for name in workers:  # one unrecorded pass: every leg's first stream pays for what is left to warm
            stream(workers[name], imgs)
        res = {name: [] for name in workers}
        for rep in range(reps):
            for name in workers:
                res[name].append(stream(workers[name], imgs))
                print(f"repetition {rep}, keep_mask {name}: {res[name][-1][0]:.1f} frames/s", flush=True)
    finally:
        for w in workers.values():
            w.close()
    say(f"(2) 5 x 4 through the class (worker process, PIL in / PIL out, 512 x 512, 4 steps, ControlNet; {n_frames} frames per repetition, "
        f"{(LANES + 1) * BATCH} outstanding), legs taking turns:")
    fps = {name: [r[0] for r in res[name]] for name in res}
    for name in res:
        say(f"  keep_mask {name}: {', '.join(f'{v:.1f}' for v in fps[name])} frames/s (median {statistics.median(fps[name]):.1f}, spread {min(fps[name]):.1f} .. "
            f"{max(fps[name]):.1f}); frames per launch {', '.join(f'{r[1]:.2f}' for r in res[name])}")
    off = fps["off"]
    floor = max(off) - min(off)
    say(f"  noise floor = spread of the off repetitions = {floor:.1f} frames/s")
    for name in list(res)[1:]:
        on = fps[name]
        diff = statistics.median(on) - statistics.median(off)
        per_frame = 1e6 / statistics.median(on) - 1e6 / statistics.median(off)
        say(f"  {name} against off: {statistics.median(on) / statistics.median(off):.3f} x ({diff:+.1f} frames/s at the medians): "
            f"{'ABOVE' if abs(diff) > floor else 'within'} the noise floor; {per_frame:+.1f} us per frame ({1e6 / statistics.median(off):.0f} us per frame off)")
    if ops_us:
        est = (ops_us.get("mask_latent", 0) + OPTS["steps"] * ops_us.get("latent_keep, step form, table noise", 0) + ops_us.get("latent_keep, final form", 0)
               + ops_us.get("mask_blend, half masks", 0))
        say(f"  the {OPTS['steps']} + 3 launches of a 5-frame launch are {est:.1f} us by (1), {est / BATCH:.1f} us per frame")


def main():
    import torch

    if "--op" in sys.argv:
        return op_loop()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/keep_mask.py needs a GPU")
    say("Keep-mask stages (mask_latent, steps + 1 latent_keep, mask_blend per launch) and the stream with the switch off, on with all-255 masks, on with a half mask")
    frame_rates(kernel_times())
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
