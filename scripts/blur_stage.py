"""What the device Gaussian blur (VideoSDPipeline(edge_blur=..., mask_feather=...); include/vsd.h THE BLUR CONTRACT; csrc/blur.hip)
costs, in ONE run.  Writes profiles/blur_stage.txt.
  (a) the kernel at five 512 x 512 frames per call, per call between device events (calls back to back on one stream: the kernel and the
      gap behind it), in a child process of this script: `gauss_blur` with C = 3 and C = 1 at R = 3, 5, 15 and 32, beside `mask_blend`
      on the same buffers as the bandwidth yardstick, next to the bytes a call must move.
  (b) the stream: BASELINE.json configs[1] (512 x 512, 4 steps, ControlNet) through the drop-in class at the bench's operating point --
      worker mode, up to 5 frames per launch, 4 launch lanes -- with `edge_blur` off / on, and, on keep-mask workers with a half mask,
      `mask_feather` off / on; the repetitions of a pair's two legs taking turns, one pair after the other.  Each on leg is reported
      against its off leg, with the spread between that leg's repetitions as the noise floor.
Every GPU step is a child process under a time limit of its own (the op loop: `subprocess` timeout; every worker call: `call_timeout`);
after a step that failed nothing more is started on the card.
Run on the GPU box:
    python scripts/blur_stage.py [--reps 3] [--frames 160] [--out profiles/blur_stage.txt]
    python scripts/blur_stage.py --op            (what the child runs: 200 calls per case, back to back on one stream)"""
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
out_path = arg("--out", os.path.join(ROOT, "profiles", "blur_stage.txt"))
lines = []

BATCH, LANES = 5, 4
OPTS = dict(height=512, width=512, steps=4, prompt="pixar, cg", strength=0.6, controlnet_scale=1.0)
MODEL = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0)
H = W = 512
OP_CALLS = 200
EDGE_SIGMA, FEATHER_SIGMA = 1.4, 4.0


def say(s):
    print(s, flush=True)
    lines.append(s)


def half_mask(h, w):
    m = np.full((h, w), 255, np.uint8)
    m[:, :w // 2] = 0
    return m


def tables():
    """radius -> a valid table: Gaussians of sigma 1.0, 1.4 and 5.0 (R = 3, 5, 15) and a flat table at the largest radius"""
    from videosd_amd import blur as BL

    flat = np.zeros(BL.TAPS, np.int32)
    flat[0], flat[2:] = 32, BL.ONE // 65
    flat[1] = BL.ONE - 64 * (BL.ONE // 65)
    t = {3: BL.gauss_taps(1.0), 5: BL.gauss_taps(1.4), 15: BL.gauss_taps(5.0), 32: BL.check_taps(flat)}
    assert [int(v[0]) for v in t.values()] == list(t)
    return t


def op_loop():
    """per case OP_CALLS calls back to back; prints the time per call between device events"""
    import torch

    from videosd_amd.ops import HipOps

    ops = HipOps(0)
    dev = ops.device
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.integers(0, 256, (BATCH, H, W, 3), dtype=np.uint8)).to(dev)
    dst = torch.from_numpy(rng.integers(0, 256, (BATCH, H, W, 3), dtype=np.uint8)).to(dev)
    mask = torch.from_numpy(np.broadcast_to(half_mask(H, W), (BATCH, H, W)).copy()).to(dev)
    soft = torch.zeros_like(mask)
    taps = {r: torch.from_numpy(t).to(dev) for r, t in tables().items()}
    rgb_mb = BATCH * H * W * 3 / 1e6
    cases = [("mask_blend, half masks (the yardstick)", lambda: ops.mask_blend(src, dst, mask, BATCH, H, W), f"{3 * rgb_mb + rgb_mb / 3:.2f} MB")]
    for r, t in taps.items():
        cases.append((f"gauss_blur, C = 3, R = {r}", lambda t=t: ops.gauss_blur(src, dst, BATCH, H, W, 3, t), f"{2 * rgb_mb:.2f} MB"))
    for r, t in taps.items():
        cases.append((f"gauss_blur, C = 1, R = {r}", lambda t=t: ops.gauss_blur(mask, soft, BATCH, H, W, 1, t), f"{2 * rgb_mb / 3:.2f} MB"))
    torch.cuda.synchronize()
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
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--op"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:  # (possibly a fault on the card: nothing more is started on it)
        raise SystemExit(f"(a) the op loop failed (exit {r.returncode}): {r.stderr[-400:]}")
    say(f"(a) per call between device events, five {W} x {H} frames per call ({OP_CALLS} calls back to back on one stream: the kernel and the gap behind it):")
    for ln in r.stdout.splitlines():
        if ln.startswith("op "):
            say("  " + ln[3:])


def worker(kw, mask):
    from videosd_amd.pipeline import VideoSDPipeline

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


def frame_rates():
    from PIL import Image

    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:512, 0:512]
    imgs = [Image.fromarray((rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) // 2 + ((xx * 2 + yy + 17 * i) % 256).astype(np.uint8)[..., None] // 2), "RGB")
            for i in range(8)]  # (bench.py's synthetic frames: seeded noise blended with a moving gradient)
    mask = half_mask(360, 640)  # (a mask of another size: sized once per plan size)
    legs = {"off": ({}, None), f"edge_blur={EDGE_SIGMA}": (dict(edge_blur=EDGE_SIGMA), None),
            "keep_mask, half mask": (dict(keep_mask=True), mask), f"keep_mask, half mask, mask_feather={FEATHER_SIGMA}": (dict(keep_mask=True, mask_feather=FEATHER_SIGMA), mask)}
    pairs = [("off", f"edge_blur={EDGE_SIGMA}"), ("keep_mask, half mask", f"keep_mask, half mask, mask_feather={FEATHER_SIGMA}")]
    res = {name: [] for name in legs}
    for pair in pairs:  # (the two workers of a pair alive at a time: four SD1.5 workers at 5 x 4 ran out of device memory)
        workers = {}
        try:
            for name in pair:
                t0 = time.perf_counter()
                workers[name] = worker(*legs[name])
                print(f"worker {name}: loaded and warmed in {time.perf_counter() - t0:.0f} s", flush=True)
            for name in workers:  # one unrecorded pass: every leg's first stream pays for what is left to warm
                stream(workers[name], imgs)
            for rep in range(reps):
                for name in workers:
                    res[name].append(stream(workers[name], imgs))
                    print(f"repetition {rep}, {name}: {res[name][-1][0]:.1f} frames/s", flush=True)
        finally:
            for w in workers.values():
                w.close()
    say(f"(b) 5 x 4 through the class (worker process, PIL in / PIL out, 512 x 512, 4 steps, ControlNet; {n_frames} frames per repetition, "
        f"{(LANES + 1) * BATCH} outstanding), the two legs of a pair taking turns:")
    fps = {name: [r[0] for r in res[name]] for name in res}
    for name in res:
        say(f"  {name}: {', '.join(f'{v:.1f}' for v in fps[name])} frames/s (median {statistics.median(fps[name]):.1f}, spread {min(fps[name]):.1f} .. "
            f"{max(fps[name]):.1f}); frames per launch {', '.join(f'{r[1]:.2f}' for r in res[name])}")
    for off_name, on_name in pairs:
        off, on = fps[off_name], fps[on_name]
        floor = max(off) - min(off)
        diff = statistics.median(on) - statistics.median(off)
        per_frame = 1e6 / statistics.median(on) - 1e6 / statistics.median(off)
        say(f"  {on_name} against {off_name}: {statistics.median(on) / statistics.median(off):.3f} x ({diff:+.1f} frames/s at the medians; noise floor = spread of "
            f"the off repetitions = {floor:.1f}): {'ABOVE' if abs(diff) > floor else 'within'} the noise floor; {per_frame:+.1f} us per frame "
            f"({1e6 / statistics.median(off):.0f} us per frame off)")


def main():
    import torch

    if "--op" in sys.argv:
        return op_loop()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/blur_stage.py needs a GPU")
    say("The device Gaussian blur (one gauss_blur per launch and switch) and the stream with edge_blur off / on and, on keep-mask workers, mask_feather off / on")
    kernel_times()
    frame_rates()
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
