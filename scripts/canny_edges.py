"""What the Canny edge stage (VideoSDPipeline(edges="canny"); include/vsd.h THE EDGE CONTRACT; csrc/canny.hip) costs beside the default
Sobel stand-in, in ONE run.  Writes profiles/canny_edges.txt.
  (1) kernel times: device time of the four canny launches next to sobel_max + sobel_apply, by kernel trace (a child process of this
      script under `rocprofv3 --kernel-trace`, no counters in that run), at 512 x 512 and 1080 x 1080, on the dense frame of the tests
      (a sine pattern under noise: about a third of all pixels are candidates) and on a smooth one;
  (2) frame rate: BASELINE configs[1] (SD1.5 + ControlNet + TAESD, 512 x 512, 4 steps) through the drop-in class -- a worker process per
      mode, up to 5 frames per launch, 4 launch lanes -- with edges="sobel" and edges="canny", three repetitions each, taking turns.  The
      canny leg is reported against the sobel leg of the same run, with the spread between the sobel repetitions as the noise floor.
The acceptance is the table, not a target: the mode is opt-in and the default program is untouched.  Needs a GPU.
    python scripts/canny_edges.py [--reps 3] [--frames 160] [--out profiles/canny_edges.txt]
    python scripts/canny_edges.py --op            (what the child runs: 200 calls of each op per frame, back to back on one stream)"""
import asyncio
import collections
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps, n_frames = int(arg("--reps", "3")), int(arg("--frames", "160"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "canny_edges.txt"))
lines = []

BATCH, LANES = 5, 4
OPTS = dict(height=512, width=512, steps=4, prompt="pixar, cg", strength=0.6, controlnet_scale=1.0)
MODEL = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0)
THR = (100, 200)
SIZES = ((512, 512), (1080, 1080))
OP_CALLS = 200
TILE_W, TILE_H = 32, 16  # csrc/canny_core.h
KERNELS = ("sobel_max", "sobel_apply", "canny_tile", "canny_border", "canny_mark", "canny_write")


def say(s):
    print(s, flush=True)
    lines.append(s)


def frame(kind, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0)
    if kind == "dense":  # (tests/canny_cases.py noise_frame)
        return np.clip(base[..., None] + np.random.default_rng(0).normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
    return np.repeat(np.clip(127 + 100 * np.sin(xx / 37.0) * np.cos(yy / 29.0), 0, 255).astype(np.uint8)[..., None], 3, axis=2)  # smooth


def op_loop():
    """the child under the profiler: per size and frame, OP_CALLS calls of each op"""
    import torch

    from videosd_amd.ops import HipOps

    ops = HipOps(0)
    for h, w in SIZES:
        for kind in ("dense", "smooth"):
            f = torch.from_numpy(frame(kind, h, w)).to(ops.device)
            edge = torch.zeros(h * w, dtype=torch.uint8, device=ops.device)
            ctrl = torch.zeros(h * w, 8, dtype=torch.float16, device=ops.device)
            for _ in range(OP_CALLS):
                ops.sobel_control(f, h, w, 0.11, 0.8, edge, ctrl)
            ops.synchronize()
            for _ in range(OP_CALLS):
                ops.canny_control(f, h, w, THR[0], THR[1], edge, ctrl)
            ops.synchronize()
            print(f"op {h}x{w} {kind}: {int((edge > 0).sum())} edge pixels of {h * w}", flush=True)


def kernel_times():
    """(1): run `--op` under the kernel trace, group the trace by kernel and frame (the calls come in a known order)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--op"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        for ln in r.stdout.splitlines():
            if ln.startswith("op "):
                say("  " + ln)
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not traces:
            say(f"(1) kernel trace: the profiled child failed (exit {r.returncode}, {len(traces)} trace files): {r.stderr[-400:]}")
            return
        rows = []
        for t in traces:
            rows += [x for x in csv.DictReader(open(t)) if any(k in x.get("Kernel_Name", "") for k in KERNELS)]
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    per = collections.defaultdict(list)  # kernel -> durations in call order
    for x in rows:
        name = next(k for k in KERNELS if k in x["Kernel_Name"])
        per[name].append((int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3)
    cases = [(h, w, kind) for h, w in SIZES for kind in ("dense", "smooth")]
    if any(len(per[k]) != OP_CALLS * len(cases) for k in KERNELS):
        say(f"(1) kernel trace: unexpected launch counts {dict((k, len(v)) for k, v in per.items())}")
        return
    say(f"(1) device time per launch, microseconds, median of {OP_CALLS} back-to-back calls (min in brackets), rocprofv3 --kernel-trace:")
    say(f"  {'frame':>18} " + " ".join(f"{k:>13}" for k in KERNELS) + f" {'sobel sum':>10} {'canny sum':>10}")
    for i, (h, w, kind) in enumerate(cases):
        med = {k: statistics.median(per[k][i * OP_CALLS:(i + 1) * OP_CALLS]) for k in KERNELS}
        mn = {k: min(per[k][i * OP_CALLS:(i + 1) * OP_CALLS]) for k in KERNELS}
        say(f"  {f'{w}x{h} {kind}':>18} " + " ".join(f"{f'{med[k]:.1f} ({mn[k]:.1f})':>13}" for k in KERNELS) +
            f" {med['sobel_max'] + med['sobel_apply']:>10.1f} {sum(med[k] for k in KERNELS[2:]):>10.1f}")
    say("  (the sums are kernel time only: a call's launches run back to back on one stream, the gaps between them are not in it)")
    return {k: statistics.median(per[k][:OP_CALLS]) for k in KERNELS}  # the first case: 512 x 512, dense


def worker(edges):
    from videosd_amd.pipeline import VideoSDPipeline

    w = VideoSDPipeline.remote(batch=BATCH, lanes=LANES, shm_slots=(LANES + 1) * BATCH + 4, call_timeout=600.0, edges=edges, canny_thresholds=THR, **MODEL)
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


def frame_rates(med):
    from PIL import Image

    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:512, 0:512]
    imgs = [Image.fromarray((rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) // 2 + ((xx * 2 + yy + 17 * i) % 256).astype(np.uint8)[..., None] // 2), "RGB")
            for i in range(8)]  # (bench.py's synthetic frames: seeded noise blended with a moving gradient)
    workers = {}
    try:
        for m in ("sobel", "canny"):
            t0 = time.perf_counter()
            workers[m] = worker(m)
            print(f"worker edges={m}: loaded and warmed in {time.perf_counter() - t0:.0f} s", flush=True)
        for m in workers:  # one unrecorded pass: every leg's first stream pays for what is left to warm
            stream(workers[m], imgs)
        res = {m: [] for m in workers}
        for rep in range(reps):
            for m in workers:
                res[m].append(stream(workers[m], imgs))
                print(f"repetition {rep}, edges={m}: {res[m][-1][0]:.1f} frames/s", flush=True)
    finally:
        for w in workers.values():
            w.close()
    say(f"(2) 5 x 4 through the class (worker process, PIL in / PIL out, 512 x 512, 4 steps, ControlNet; {n_frames} frames per repetition, "
        f"{(LANES + 1) * BATCH} outstanding), legs taking turns:")
    fps = {m: [r[0] for r in res[m]] for m in res}
    for m in res:
        say(f"  edges={m}: {', '.join(f'{v:.1f}' for v in fps[m])} frames/s (median {statistics.median(fps[m]):.1f}, spread {min(fps[m]):.1f} .. {max(fps[m]):.1f}); "
            f"frames per launch {', '.join(f'{r[1]:.2f}' for r in res[m])}")
    s, c = fps["sobel"], fps["canny"]
    floor = max(s) - min(s)
    diff = statistics.median(c) - statistics.median(s)
    say(f"  canny against sobel: {statistics.median(c) / statistics.median(s):.3f} x ({diff:+.1f} frames/s at the medians); noise floor = spread of the sobel "
        f"repetitions = {floor:.1f} frames/s: the difference is {'ABOVE' if abs(diff) > floor else 'within'} the noise floor")
    if med:
        # what the stage costs, and which launch: a frame of the stream takes 1 / (frames/s); the stage's kernel time per frame is in (1)
        extra = sum(med[k] for k in KERNELS[2:]) - med["sobel_max"] - med["sobel_apply"]
        per_frame = 1e6 / statistics.median(c) - 1e6 / statistics.median(s)
        shares = sorted(((med[k], k) for k in KERNELS[2:]), reverse=True)
        say(f"  a frame of the canny stream takes {per_frame:+.1f} us against the sobel stream ({1e6 / statistics.median(s):.0f} us per frame); the canny launches are "
            f"{extra:+.1f} us of kernel time per 512 x 512 dense frame beside the two sobel launches, and two launches more per frame; "
            f"largest first: {', '.join(f'{k} {v:.1f} us' for v, k in shares)}")


def main():
    import torch

    if "--op" in sys.argv:
        return op_loop()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/canny_edges.py needs a GPU")
    say(f"Canny edge stage beside the Sobel stand-in; thresholds {THR}; tile {TILE_W} x {TILE_H}")
    frame_rates(kernel_times())
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
