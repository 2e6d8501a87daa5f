"""Per-frame prompts (VideoSDPipeline(frame_prompts=True); Engine.prepare(frame_prompts=True); include/vsd.h vsd_prompt_install), measured on
BASELINE configs[1] (SD1.5 + ControlNet + TAESD, 512x512, 4 steps) through the drop-in class: a worker process, up to 5 frames per launch,
4 launch lanes.
  (a) one prompt everywhere: the default program beside the frame_prompts program -- what the explicit cross-attention at the 640- and
      1280-wide levels costs against the absorbed form;
  (b) five sessions with five prompts: frame i carries prompt i mod 5.  Without frame_prompts a launch has one prompt (such frames never share
      one), with it they coalesce; frames/s and the p50 of a frame's latency (request sent -> reply);
  (c) the device time of one vsd_prompt_install (one changed frame slot of a 5-frame block), between events.
The legs of (a) and (b) take turns, three repetitions each, in ONE run.  Needs a GPU.
    python scripts/frame_prompts.py [--reps 3] [--frames 160] [--out profiles/frame_prompts.txt]"""
import asyncio
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videosd_amd.pipeline import VideoSDPipeline  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps, n_frames = int(arg("--reps", "3")), int(arg("--frames", "160"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "frame_prompts.txt"))
lines = []

BATCH, LANES = 5, 4
OPTS = dict(height=512, width=512, strength=0.6, steps=4, controlnet_scale=1.0)
PROMPTS = ["pixar, cg", "a watercolor painting", "a charcoal sketch", "oil on canvas, impasto", "neon city at night"]
MODEL = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0)


def say(s):
    print(s, flush=True)
    lines.append(s)


def worker(frame_prompts):
    w = VideoSDPipeline.remote(batch=BATCH, lanes=LANES, shm_slots=(LANES + 1) * BATCH + 4, call_timeout=600.0, max_prompts=16,
                               frame_prompts=frame_prompts, **MODEL)
    w.method("warm_up")(batches=tuple(range(1, BATCH + 1)), lanes=LANES, prompt=PROMPTS[0], **OPTS)
    return w


def stream(w, imgs, prompts):
    """`n_frames` frames, (LANES + 1) * BATCH outstanding, frame i with prompts[i mod len] -> (frames/s, p50 latency ms, frames per launch)"""
    before = w.metrics()
    lat = []

    async def go():
        sem = asyncio.Semaphore((LANES + 1) * BATCH)

        async def one(i):
            async with sem:
                t = time.perf_counter()
                await w.infer.remote(imgs[i % len(imgs)], prompt=prompts[i % len(prompts)], **OPTS)
                lat.append(time.perf_counter() - t)

        t0 = time.perf_counter()
        await asyncio.gather(*[one(i) for i in range(n_frames)])
        return n_frames / (time.perf_counter() - t0)

    fps = asyncio.run(go())
    after = w.metrics()
    launches = after["launches"] - before["launches"]
    return fps, 1e3 * float(np.median(lat)), (after["frames"] - before["frames"]) / max(launches, 1)


def install_cost():
    """(c): one cache entry into one slot of a 5-frame block of the real networks, 200 launches between two events"""
    p = VideoSDPipeline(frame_prompts=True, tuning_mode="table", **MODEL)
    eng = p.model
    from videosd_amd.engine import FramePromptLayout, PromptBlock

    blk = eng.build_prompt(p.encode_prompt(PROMPTS[1]))
    lay = FramePromptLayout(eng._nets(), blk.layout.tl, BATCH)
    dst = PromptBlock(eng.ops, lay)
    tab, nseg = eng._seg_table(blk.layout, lay)
    nbytes = sum(int(r) * int(rb) for _so, _do, r, rb, _p, _f in tab.cpu().tolist())
    ops = eng.ops
    for f in range(BATCH):
        ops.prompt_install(blk.buf, dst.buf, tab, nseg, f)
    ops.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ops.stream)
        for i in range(200):
            ops.prompt_install(blk.buf, dst.buf, tab, nseg, i % BATCH)
        e1.record(ops.stream)
        ops.synchronize()
        ms.append(e0.elapsed_time(e1) / 200)
    med = float(np.median(ms))
    say(f"(c) vsd_prompt_install, one slot of a {BATCH}-frame block, {nseg} segments, {nbytes / 1e6:.2f} MB read + written: "
        f"{', '.join(f'{1e3 * v:.1f}' for v in ms)} us per launch (200 back to back between two events; median {1e3 * med:.1f} us, "
        f"{2 * nbytes / (med * 1e-3) / 1e9:.0f} GB/s of traffic); a single-prompt engine's switch copies its whole {blk.layout.nbytes / 1e6:.1f} MB block")


def main():
    from PIL import Image

    if not torch.cuda.is_available():
        raise SystemExit("scripts/frame_prompts.py needs a GPU")
    rng = np.random.default_rng(0)
    imgs = [Image.fromarray(rng.integers(0, 256, (512, 512, 3), dtype=np.uint8), "RGB") for _ in range(8)]
    workers = {False: worker(False), True: worker(True)}
    try:
        legs = [("(a) one prompt, frame_prompts off (the default program)", False, PROMPTS[:1]),
                ("(a) one prompt, frame_prompts on", True, PROMPTS[:1]),
                ("(b) five prompts, frame_prompts off (a launch has one prompt)", False, PROMPTS),
                ("(b) five prompts, frame_prompts on", True, PROMPTS)]
        for name, fp, prompts in legs:  # one unrecorded pass: every leg's first stream pays for what is left to warm
            stream(workers[fp], imgs, prompts)
        res = {name: [] for name, _f, _p in legs}
        for _ in range(reps):
            for name, fp, prompts in legs:
                res[name].append(stream(workers[fp], imgs, prompts))
        say(f"5 x 4 through the class (worker process, PIL in / PIL out, {n_frames} frames per repetition, {(LANES + 1) * BATCH} outstanding), legs taking turns:")
        med = {}
        for name, _f, _p in legs:
            fps = [r[0] for r in res[name]]
            med[name] = (float(np.median(fps)), min(fps), max(fps))
            say(f"  {name}: {', '.join(f'{v:.1f}' for v in fps)} frames/s (median {med[name][0]:.1f}, spread {min(fps):.1f} .. {max(fps):.1f}); "
                f"p50 latency {', '.join(f'{r[1]:.0f}' for r in res[name])} ms; frames per launch {', '.join(f'{r[2]:.2f}' for r in res[name])}")
        (a_off, a_on), (b_off, b_on) = [med[n] for n, _f, _p in legs[:2]], [med[n] for n, _f, _p in legs[2:]]
        say(f"(a) frame_prompts on / off with one prompt: {a_on[0] / a_off[0]:.3f} x")
        say(f"(b) frame_prompts on / off with five prompts: {b_on[0] / b_off[0]:.3f} x; "
            f"{'on beats off by more than the spread' if b_on[1] > b_off[2] else 'NOT separated by more than the spread of the repetitions'} "
            f"(slowest on {b_on[1]:.1f}, fastest off {b_off[2]:.1f})")
    finally:
        for w in workers.values():
            w.close()
    install_cost()
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
