"""Prompt mixes (include/vsd.h THE PROMPT MIX; `prompt={"mix": [[text, weight], ...]}`), measured on BASELINE configs[1] (SD1.5 + ControlNet +
TAESD, 512x512, 4 steps; synthetic weights where no checkpoint is installed):
  (a) the device time of one vsd_prompt_mix over the full prompt block at n = 2 and n = 4, beside the device-to-device block copy it
      replaces, with the bytes moved over that time -- between events here (200 launches back to back), and from a kernel trace when the
      leg is run under rocprofv3 and folded in (below);
  (b) the 5 x 4 stream through the class (a worker process, up to 5 frames per launch, 4 launch lanes) with a NEW mix value on every
      launch, against the same stream with a fixed prompt and against the same sweep done the only way it could be done before mixes:
      host-blended embeddings through `set_prompt_embeds`, one new cache entry per value (that path is unchanged by this feature);
      frames/s, p50 latency, and the prompt builds and their host time from `metrics()`;
  (c) a `frame_prompts` worker: five sessions with five plain prompts, with five fixed mixes, and with five mixes that each move on
      every frame.
The legs of (b) and of (c) take turns, `--reps` repetitions each, in ONE run.  Needs a GPU.
    python scripts/prompt_mix.py [--reps 3] [--frames 160] [--out profiles/prompt_mix.txt]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/prompt_mix.py --only-a --launches 20
    python scripts/prompt_mix.py --fold-trace DIR [--out profiles/prompt_mix.txt]      (appends the kernel times of that trace)"""
import asyncio
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videosd_amd import promptmix as PM  # noqa: E402
from videosd_amd.pipeline import VideoSDPipeline  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps, n_frames, n_launches = int(arg("--reps", "3")), int(arg("--frames", "160")), int(arg("--launches", "200"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "prompt_mix.txt"))
lines = []

BATCH, LANES = 5, 4
OUTSTANDING = (LANES + 1) * BATCH
OPTS = dict(height=512, width=512, strength=0.6, steps=4, controlnet_scale=1.0)
PROMPTS = ["pixar, cg", "a watercolor painting", "a charcoal sketch", "oil on canvas, impasto", "neon city at night"]
TEXT_A, TEXT_B = PROMPTS[1], PROMPTS[2]
MODEL = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0)
SWEEP = 64  # mix values of a sweep before it turns round


def say(s):
    print(s, flush=True)
    lines.append(s)


def mix(k):
    """value k of the sweep between TEXT_A and TEXT_B: a triangle wave over SWEEP positions, never an end point"""
    t = (abs(k % (2 * SWEEP) - SWEEP) + 0.5) / (SWEEP + 1)
    return {"mix": [[TEXT_A, 1.0 - t], [TEXT_B, t]]}


# ------------------------------------------------------------------------------------------ (a) the kernel
def mix_cost(trace_only=False):
    p = VideoSDPipeline(tuning_mode="table", **MODEL)
    eng = p.model
    from videosd_amd.blocks import PromptBlock

    blks = [eng.build_prompt(p.encode_prompt(t)) for t in PROMPTS[:4]]
    lay = blks[0].layout
    dst = PromptBlock(eng.ops, lay)
    tab, nseg = eng._seg_table(lay, lay, mix=True)
    ops = eng.ops
    legs = [("copy_ (the plain prompt's block copy)", 1, lambda: ops.copy_(dst.buf, blks[0].buf))]
    for n in (2, 4):
        ws = PM.normalized([1.0 + i for i in range(n)])
        legs.append((f"vsd_prompt_mix n = {n}", n, lambda n=n, ws=ws: ops.prompt_mix([b.buf for b in blks[:n]], ws, dst.buf, tab, nseg, 0)))
    if not trace_only:
        say(f"(a) one prompt block of SD1.5 + ControlNet: {lay.nbytes / 1e6:.2f} MB in {nseg} segments; {n_launches} launches back to back between two "
            "events, five repetitions")
    for name, n, fn in legs:
        for _ in range(3):
            fn()
        ops.synchronize()
        ms = []
        for _ in range(1 if trace_only else 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ops.stream)
            for _i in range(n_launches):
                fn()
            e1.record(ops.stream)
            ops.synchronize()
            ms.append(e0.elapsed_time(e1) / n_launches)
        med = float(np.median(ms))
        moved = (n + 1) * lay.nbytes
        if not trace_only:
            say(f"  {name}: {', '.join(f'{1e3 * v:.1f}' for v in ms)} us per launch (median {1e3 * med:.1f} us); {moved / 1e6:.1f} MB read + written: "
                f"{moved / (med * 1e-3) / 1e9:.0f} GB/s")
    return lay.nbytes


def fold_trace(directory):
    """the kernel times of a rocprofv3 --kernel-trace of `--only-a`, appended to the profile"""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    per = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            # (the copy kernel also moves the 640-byte biases of every prompt build: only copies of more than 10 us are block copies)
            if "prompt_mix_kernel" in name or ("copyBuffer" in name and us > 10.0):
                per.setdefault(name, []).append(us)
    out = ["(a) by kernel trace (rocprofv3 --kernel-trace of `--only-a`; device time of every launch of the kernel, warm-up launches included):"]
    for name, us in sorted(per.items()):
        short = name if len(name) < 90 else name[:87] + "..."
        out.append(f"  {short}: {len(us)} launches, median {float(np.median(us)):.1f} us, min {min(us):.1f}, max {max(us):.1f}")
    if len(out) == 1:
        out.append("  (no prompt_mix or copyBuffer kernel in the trace)")
    for s in out:
        print(s)
    with open(out_path, "a") as fh:
        fh.write("\n".join(out) + "\n")


# ------------------------------------------------------------------------------------------ (b), (c) streams through a worker
def worker(frame_prompts):
    w = VideoSDPipeline.remote(batch=BATCH, lanes=LANES, shm_slots=OUTSTANDING + 4, call_timeout=600.0, frame_prompts=frame_prompts, **MODEL)
    w.method("warm_up")(batches=tuple(range(1, BATCH + 1)), lanes=LANES, prompt=TEXT_A, **OPTS)
    w.infer(IMGS[0], prompt=TEXT_B, **OPTS)  # (both texts of the sweep are cached before anything is timed)
    return w


def stream(w, prompt_of, before_frame=None):
    """`n_frames` frames sent in order, OUTSTANDING of them outstanding, frame i with prompt_of(i); before_frame(i) may post another call ahead
    of frame i -> (frames/s, p50 latency ms, frames per launch, prompt builds, median build ms)"""
    before = w.metrics()
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
            if before_frame is not None:
                before_frame(i)
            tasks.append(asyncio.ensure_future(one(w.infer.remote(IMGS[i % len(IMGS)], prompt=prompt_of(i), **OPTS), time.perf_counter())))
        await asyncio.gather(*tasks)
        return n_frames / (time.perf_counter() - t0)

    fps = asyncio.run(go())
    after = w.metrics()
    launches = after["launches"] - before["launches"]
    pa, pb = after["pipeline"]["stage_ms_p50"], before["pipeline"]["stage_ms_p50"]
    return fps, 1e3 * float(np.median(lat)), (after["frames"] - before["frames"]) / max(launches, 1), pa["prompt_builds"] - pb["prompt_builds"], pa["prompt"]


def run_legs(title, w, legs):
    for _name, prompt_of, pre in legs:  # one unrecorded pass: every leg's first stream pays for what is left to warm
        stream(w, prompt_of, pre)
    res = {name: [] for name, _p, _b in legs}
    for _ in range(reps):
        for name, prompt_of, pre in legs:
            res[name].append(stream(w, prompt_of, pre))
    say(title)
    med = {}
    for name, _p, _b in legs:
        fps = [r[0] for r in res[name]]
        med[name] = (float(np.median(fps)), min(fps), max(fps))
        say(f"  {name}: {', '.join(f'{v:.1f}' for v in fps)} frames/s (median {med[name][0]:.1f}, spread {min(fps):.1f} .. {max(fps):.1f}); "
            f"p50 latency {', '.join(f'{r[1]:.0f}' for r in res[name])} ms; frames per launch {', '.join(f'{r[2]:.2f}' for r in res[name])}; "
            f"prompt builds {', '.join(str(r[3]) for r in res[name])} (median host time of a build {res[name][-1][4]} ms)")
    return med


def sweep_legs(w):
    """(b): a plain worker.  The frames of one launch share a mix value (frames that differ in `prompt` do not share a launch here)"""
    emb = [w.method("encode_prompt")(t).float() for t in (TEXT_A, TEXT_B)]
    run = [0]

    def blended(i):
        """the way of the parent commit: value k as host-blended embeddings under a key of its own, posted ahead of its first frame"""
        if i % BATCH == 0:
            k = i // BATCH
            wa, wb = PM.canonical(mix(k)).weights
            w.set_prompt_embeds.remote((wa * emb[0] + wb * emb[1]).half(), key=f"sweep {run[0]} {k}")
        if i == n_frames - 1:
            run[0] += 1

    legs = [("fixed prompt", lambda i: TEXT_A, None),
            ("a new mix value on every launch", lambda i: mix(i // BATCH), None),
            ("the same sweep as host-blended embeddings through set_prompt_embeds", lambda i: f"sweep {run[0]} {i // BATCH}", blended)]
    med = run_legs(f"(b) 5 x 4 through the class (worker process, PIL in / PIL out, {n_frames} frames per repetition, {OUTSTANDING} outstanding), legs "
                   "taking turns:", w, legs)
    fixed, swept, old = (med[n] for n, _p, _b in legs)
    say(f"(b) mix sweep / fixed prompt: {swept[0] / fixed[0]:.3f} x "
        f"({'NOT ' if swept[2] >= fixed[1] else ''}separated by more than the spread: fastest sweep {swept[2]:.1f}, slowest fixed {fixed[1]:.1f}); "
        f"mix sweep / blended embeddings: {swept[0] / old[0]:.3f} x (slowest sweep {swept[1]:.1f}, fastest blended {old[2]:.1f})")


def session_legs(w):
    """(c): a `frame_prompts` worker, frame i belongs to session i mod 5"""
    pairs = [(PROMPTS[s], PROMPTS[(s + 1) % 5]) for s in range(5)]
    for t in PROMPTS:
        w.infer(IMGS[0], prompt=t, **OPTS)

    def fixed(i):
        a, b = pairs[i % 5]
        return {"mix": [[a, 0.3 + 0.1 * (i % 5)], [b, 0.7 - 0.1 * (i % 5)]]}

    def moving(i):
        a, b = pairs[i % 5]
        t = (abs((i // 5) % (2 * SWEEP) - SWEEP) + 0.5) / (SWEEP + 1)
        return {"mix": [[a, 1.0 - t], [b, t]]}

    legs = [("five sessions, five plain prompts", lambda i: PROMPTS[i % 5], None), ("five sessions, five fixed mixes", fixed, None),
            ("five sessions, each mix moving on every frame", moving, None)]
    med = run_legs(f"(c) a frame_prompts worker, 5 x 4, {n_frames} frames per repetition, legs taking turns:", w, legs)
    plain, fx, mv = (med[n] for n, _p, _b in legs)
    say(f"(c) fixed mixes / plain prompts: {fx[0] / plain[0]:.3f} x; moving mixes / plain prompts: {mv[0] / plain[0]:.3f} x "
        f"(slowest moving {mv[1]:.1f}, slowest plain {plain[1]:.1f} frames/s)")


IMGS = []


def main():
    from PIL import Image

    if "--fold-trace" in sys.argv:
        return fold_trace(arg("--fold-trace", ""))
    if not torch.cuda.is_available():
        raise SystemExit("scripts/prompt_mix.py needs a GPU")
    if "--only-a" in sys.argv:
        mix_cost(trace_only=True)
        return
    rng = np.random.default_rng(0)
    IMGS.extend(Image.fromarray(rng.integers(0, 256, (512, 512, 3), dtype=np.uint8), "RGB") for _ in range(8))
    mix_cost()
    for fp, legs in ((False, sweep_legs), (True, session_legs)):
        w = worker(fp)
        try:
            legs(w)
        finally:
            w.close()
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
