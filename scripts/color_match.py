"""What the colour-match stage (VideoSDPipeline(color_match=...); include/vsd.h THE COLOUR CONTRACT; csrc/color_match.hip) costs, in ONE run.
Writes profiles/color_match.txt.
  (1) the three launches at 512 x 512 and 1080 x 1080, one and five frames per call, both modes: per call between device events (calls back
      to back on one stream: kernels and the gaps between them), and per kernel by kernel trace (a child process of this script under
      rocprofv3), next to the bytes a call must move.
  (2) the stream: BASELINE.json configs[1] (512 x 512, 4 steps, ControlNet) through the drop-in class at the bench's operating point --
      worker mode, up to 5 frames per launch, 4 launch lanes -- with the mode off and with color_match="histogram", repetitions taking
      turns.  The off leg records the programs of the commit before (equal fingerprints); the on leg is reported against it, with the spread
      between the off repetitions as the noise floor.
Run on the GPU box:
    python scripts/color_match.py [--reps 3] [--frames 160] [--out profiles/color_match.txt]
    python scripts/color_match.py --op            (what the child runs: 200 calls per case, back to back on one stream)"""
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
out_path = arg("--out", os.path.join(ROOT, "profiles", "color_match.txt"))
lines = []

BATCH, LANES = 5, 4
OPTS = dict(height=512, width=512, steps=4, prompt="pixar, cg", strength=0.6, controlnet_scale=1.0)
MODEL = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0)
SIZES = ((512, 512), (1080, 1080))
FRAMES = (1, 5)
MODES = ("histogram", "meanstd")
OP_CALLS = 200
KERNELS = ("color_hist", "color_lut", "color_apply")
CASES = [(h, w, f, m) for h, w in SIZES for f in FRAMES for m in MODES]


def say(s):
    print(s, flush=True)
    lines.append(s)


def picture(h, w, seed):
    """a camera-like frame and a flatter, shifted one (what a restyled frame looks like to this stage): smooth regions, so that many lanes of
    a wave count the same value -- the case LDS atomics like least"""
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    base = 127 + 100 * np.sin(xx / 37.0 + seed) * np.cos(yy / 29.0)
    src = np.clip(base[..., None] * np.array([1.0, 0.8, 0.6]) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
    dst = np.clip(40 + base[..., None] * np.array([0.5, 0.6, 0.6]) + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    return src, dst


def op_loop():
    """per case OP_CALLS calls back to back; prints the time per call between device events"""
    import torch

    from videosd_amd.ops import HipOps

    ops = HipOps(0)
    for h, w, frames, mode in CASES:
        pairs = [picture(h, w, s) for s in range(frames)]
        src = torch.from_numpy(np.stack([p[0] for p in pairs])).to(ops.device)
        dst = torch.from_numpy(np.stack([p[1] for p in pairs])).to(ops.device)
        am = torch.full((frames,), 256, dtype=torch.int32, device=ops.device)
        torch.cuda.synchronize()
        for _ in range(20):  # warm-up: code objects, the workspace
            ops.color_match(src, dst, frames, h, w, mode, am)
        ops.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ops.stream)
        for _ in range(OP_CALLS):
            ops.color_match(src, dst, frames, h, w, mode, am)
        e1.record(ops.stream)
        ops.synchronize()
        print(f"op {w}x{h} x{frames} {mode}: {e0.elapsed_time(e1) * 1e3 / OP_CALLS:.1f} us per call between events ({OP_CALLS} calls back to back)", flush=True)


def kernel_times():
    """(1): run `--op` under the kernel trace, group the trace by kernel and case (the calls come in a known order)"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--op"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:  # (possibly a fault on the card: nothing more is started on it)
        raise SystemExit(f"(1) the op loop failed (exit {r.returncode}): {r.stderr[-400:]}")
    say(f"(1a) per call between device events, profiler off (three launches and the gaps between them; {OP_CALLS} calls back to back on one stream):")
    for ln in r.stdout.splitlines():
        if ln.startswith("op "):
            say("  " + ln[3:])
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--op"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0:
            raise SystemExit(f"(1b) kernel trace: the profiled child failed (exit {r.returncode}): {r.stderr[-400:]}")
        if not traces:
            say("(1b) kernel trace: the profiler wrote no trace file")
            return None
        rows = []
        for t in traces:
            rows += [x for x in csv.DictReader(open(t)) if any(k in x.get("Kernel_Name", "") for k in KERNELS)]
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    per = collections.defaultdict(list)  # kernel -> durations in call order
    for x in rows:
        name = next(k for k in KERNELS if k in x["Kernel_Name"])
        per[name].append((int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3)
    each = OP_CALLS + 20
    if any(len(per[k]) != each * len(CASES) for k in KERNELS):
        say(f"(1b) kernel trace: unexpected launch counts {dict((k, len(v)) for k, v in per.items())}")
        return None
    say(f"(1b) device time per launch, microseconds, median of {OP_CALLS} back-to-back calls (min in brackets), rocprofv3 --kernel-trace; MB = what a call must "
        "move (src and dst read for the histograms, dst read and written by the apply):")
    say(f"  {'case':>26} " + " ".join(f"{k:>13}" for k in KERNELS) + f" {'sum':>8} {'MB':>7} {'GB/s of sum':>12}")
    first = None
    for i, (h, w, frames, mode) in enumerate(CASES):
        sl = slice(i * each + 20, (i + 1) * each)
        med = {k: statistics.median(per[k][sl]) for k in KERNELS}
        mn = {k: min(per[k][sl]) for k in KERNELS}
        total, mb = sum(med.values()), 4 * 3 * h * w * frames / 1e6
        say(f"  {f'{w}x{h} x{frames} {mode}':>26} " + " ".join(f"{f'{med[k]:.1f} ({mn[k]:.1f})':>13}" for k in KERNELS) + f" {total:>8.1f} {mb:>7.2f} {mb / total * 1e3:>12.0f}")
        if (h, w, frames, mode) == (512, 512, 5, "histogram"):
            first = med
    say("  (the sums are kernel time only; the pictures have smooth regions, so many lanes of a wave count the same value)")
    return first


def worker(mode):
    from videosd_amd.pipeline import VideoSDPipeline

    kw = {} if mode is None else dict(color_match=mode)
    w = VideoSDPipeline.remote(batch=BATCH, lanes=LANES, shm_slots=(LANES + 1) * BATCH + 4, call_timeout=600.0, **kw, **MODEL)
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
    legs = {"off": None, "histogram": "histogram"}
    workers = {}
    try:
        for name, mode in legs.items():
            t0 = time.perf_counter()
            workers[name] = worker(mode)
            print(f"worker color_match={mode}: loaded and warmed in {time.perf_counter() - t0:.0f} s", flush=True)
        for name in workers:  # one unrecorded pass: every leg's first stream pays for what is left to warm
            stream(workers[name], imgs)
        res = {name: [] for name in workers}
        for rep in range(reps):
            for name in workers:
                res[name].append(stream(workers[name], imgs))
                print(f"repetition {rep}, color_match={name}: {res[name][-1][0]:.1f} frames/s", flush=True)
    finally:
        for w in workers.values():
            w.close()
    say(f"(2) 5 x 4 through the class (worker process, PIL in / PIL out, 512 x 512, 4 steps, ControlNet; {n_frames} frames per repetition, "
        f"{(LANES + 1) * BATCH} outstanding), legs taking turns:")
    fps = {name: [r[0] for r in res[name]] for name in res}
    for name in res:
        say(f"  color_match={name}: {', '.join(f'{v:.1f}' for v in fps[name])} frames/s (median {statistics.median(fps[name]):.1f}, spread {min(fps[name]):.1f} .. "
            f"{max(fps[name]):.1f}); frames per launch {', '.join(f'{r[1]:.2f}' for r in res[name])}")
    off, on = fps["off"], fps["histogram"]
    floor = max(off) - min(off)
    diff = statistics.median(on) - statistics.median(off)
    say(f"  histogram against off: {statistics.median(on) / statistics.median(off):.3f} x ({diff:+.1f} frames/s at the medians); noise floor = spread of the off "
        f"repetitions = {floor:.1f} frames/s: the difference is {'ABOVE' if abs(diff) > floor else 'within'} the noise floor")
    per_frame = 1e6 / statistics.median(on) - 1e6 / statistics.median(off)
    tail = f"; the three launches are {sum(med.values()):.1f} us of kernel time per 5-frame call at 512 x 512 (1b)" if med else ""
    say(f"  a frame of the histogram stream takes {per_frame:+.1f} us against the off stream ({1e6 / statistics.median(off):.0f} us per frame){tail}")


def main():
    import torch

    if "--op" in sys.argv:
        return op_loop()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/color_match.py needs a GPU")
    say("Colour-match stage (three launches per call: histograms, LUT, apply) and the stream with the mode off and on")
    frame_rates(kernel_times())
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
