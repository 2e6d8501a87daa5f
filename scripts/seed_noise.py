"""Per-frame seeded noise (VideoSDPipeline(device_seed=True); include/vsd.h THE NOISE CONTRACT), measured on BASELINE configs[1] (SD1.5 +
ControlNet + TAESD, 512x512, 4 steps): how far the device's normals are from the contract evaluated in fp64, and the 5 x 4 stream through
the drop-in class (worker process, up to 5 frames per launch, 4 launch lanes) with device_seed off and on, plus streams whose frames
alternate between two seeds -- which coalesce with device_seed (one launch holds both seeds) and cannot without it (a launch has one
`seed`).  The legs take turns, three repetitions each, in ONE run: the yardstick of the device_seed legs is the device_seed=False leg
beside them.
    python scripts/seed_noise.py [--reps 3] [--frames 160] [--out profiles/seed_noise.txt]"""
import asyncio
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seed_cases as SC  # noqa: E402  (the contract in numpy)
from videosd_amd.ops import HipOps  # noqa: E402
from videosd_amd.pipeline import VideoSDPipeline  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps, n_frames = int(arg("--reps", "3")), int(arg("--frames", "160"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "seed_noise.txt"))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def normals():
    """vsd_noise_fill against the fp64 restatement: 2^20 normals per draw"""
    ops = HipOps(0)
    hw = 1 << 18
    out = ops.zeros(4, hw, dtype=torch.float32)
    worst = 0.0
    for seed, kind, draw in [(42, 0, 3), (0, 0, 0), (2 ** 64 - 1, 1, 4), (2 ** 32 + 5, 0, 1)]:
        ops.noise_fill(seed, kind, draw, hw, out)
        ops.synchronize()
        got = out.cpu().numpy().astype(np.float64)
        err = float(np.abs(got - SC.normal_draw(seed, kind, draw, hw)).max())
        worst = max(worst, err)
        say(f"normals, seed {seed} kind {kind} draw {draw}, {4 * hw} values: max |device - fp64| {err:.3e}, max |z| {np.abs(got).max():.3f}, "
            f"mean {got.mean():+.4f}, std {got.std():.4f}")
    say(f"normals: worst {worst:.3e} (the tests' bound: 8e-6 = 4 x the 1.85e-6 of the same formulas in numpy fp32)")
    ts = []
    for _ in range(20):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ops.noise_fill(42, 0, 3, 4096, out)
        ops.synchronize()
        ts.append(time.perf_counter() - t)
    say(f"vsd_noise_fill of one 512 x 512 frame's draw (4096 pixels), launch to synchronize: median {1e6 * float(np.median(ts)):.1f} us")


BATCH, LANES = 5, 4
OPTS = dict(prompt="pixar, cg", height=512, width=512, strength=0.6, steps=4, controlnet_scale=1.0)


def worker(device_seed):
    from PIL import Image  # noqa: F401

    w = VideoSDPipeline.remote(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0, batch=BATCH, lanes=LANES,
                               shm_slots=(LANES + 1) * BATCH + 4, call_timeout=600.0, device_seed=device_seed)
    w.method("warm_up")(batches=tuple(range(1, BATCH + 1)), lanes=LANES, seed=23, **OPTS)
    return w


def stream(w, imgs, seeds):
    """`n_frames` frames, (LANES + 1) * BATCH outstanding, frame i with seed seeds[i mod len] -> (frames/s, frames per launch of THIS stream)"""
    before = w.metrics()

    async def go():
        sem = asyncio.Semaphore((LANES + 1) * BATCH)

        async def one(i):
            async with sem:
                await w.infer.remote(imgs[i % len(imgs)], seed=seeds[i % len(seeds)], **OPTS)

        t0 = time.perf_counter()
        await asyncio.gather(*[one(i) for i in range(n_frames)])
        return n_frames / (time.perf_counter() - t0)

    fps = asyncio.run(go())
    after = w.metrics()
    launches = after["launches"] - before["launches"]
    return fps, (after["frames"] - before["frames"]) / max(launches, 1)


def main():
    from PIL import Image

    normals()
    rng = np.random.default_rng(0)
    imgs = [Image.fromarray(rng.integers(0, 256, (512, 512, 3), dtype=np.uint8), "RGB") for _ in range(8)]
    workers = {False: worker(False), True: worker(True)}
    try:
        legs = [("device_seed=False, one seed", False, [23]), ("device_seed=True, one seed", True, [23]),
                ("device_seed=True, seeds alternate 23 / 24", True, [23, 24]), ("device_seed=False, seeds alternate 23 / 24 (no launch can hold both)", False, [23, 24])]
        for name, ds, seeds in legs:  # one unrecorded pass: every leg's first stream pays for what is left to warm
            stream(workers[ds], imgs, seeds)
        res = {name: [] for name, _d, _s in legs}
        for _ in range(reps):
            for name, ds, seeds in legs:
                res[name].append(stream(workers[ds], imgs, seeds))
        say(f"5 x 4 stream through the class (worker process, PIL in / PIL out, {n_frames} frames per repetition, {(LANES + 1) * BATCH} outstanding), legs taking turns:")
        for name, _d, _s in legs:
            fps = [r[0] for r in res[name]]
            say(f"  {name}: {', '.join(f'{v:.1f}' for v in fps)} frames/s (median {float(np.median(fps)):.1f}, spread {min(fps):.1f} .. {max(fps):.1f}); "
                f"frames per launch {', '.join(f'{r[1]:.2f}' for r in res[name])}")
    finally:
        for w in workers.values():
            w.close()
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
