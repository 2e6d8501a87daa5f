"""Per-frame options (VideoSDPipeline(frame_options=True); Engine.prepare(frame_options=True); include/vsd.h vsd_add_noise_frames,
vsd_lcm_step_frames, vsd_groupnorm_addvec, vsd_cn_merge_frames), measured on BASELINE configs[1] (SD1.5 + ControlNet + TAESD, 512x512,
4 steps) through the drop-in class: a worker process, up to 5 frames per launch, 4 launch lanes.
  (a) one session, one (strength, controlnet_scale): the default program beside the frame_options program -- the price of the form: conv1
      without its time vector + norm2 with it, the merge pass, zero-convs of the plain epilogue class (which kernel form they got is listed);
  (b) five sessions with five (strength, controlnet_scale) pairs of one timestep count: frame i carries pair i mod 5.  Without frame_options
      a launch has one pair and a change drains the lanes; with it such frames coalesce.  Also two sessions alternating frame by frame.
      Frames/s and the p50 of a frame's latency (request sent -> reply);
  (c) the device time of one option-entry build (a new timestep tuple) and of one slot install (one changed frame of a 5-frame block).
The legs of (a) and (b) take turns, three repetitions each, in ONE run.  Needs a GPU.
    python scripts/frame_options.py [--reps 3] [--frames 160] [--out profiles/frame_options.txt]"""
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
out_path = arg("--out", os.path.join(ROOT, "profiles", "frame_options.txt"))
lines = []

BATCH, LANES = 5, 4
BASE = dict(height=512, width=512, steps=4, prompt="pixar, cg")
PAIRS = [(0.6, 1.0), (0.5, 0.4), (0.7, 1.6), (0.8, 0.7), (0.44, 2.2)]  # four timesteps each at steps = 4
MODEL = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0)


def say(s):
    print(s, flush=True)
    lines.append(s)


def worker(frame_options):
    w = VideoSDPipeline.remote(batch=BATCH, lanes=LANES, shm_slots=(LANES + 1) * BATCH + 4, call_timeout=600.0, frame_options=frame_options, **MODEL)
    w.method("warm_up")(batches=tuple(range(1, BATCH + 1)), lanes=LANES, strength=PAIRS[0][0], controlnet_scale=PAIRS[0][1], **BASE)
    return w


def stream(w, imgs, pairs):
    """`n_frames` frames, (LANES + 1) * BATCH outstanding, frame i with pairs[i mod len] -> (frames/s, p50 latency ms, frames per launch)"""
    before = w.metrics()
    lat = []

    async def go():
        sem = asyncio.Semaphore((LANES + 1) * BATCH)

        async def one(i):
            async with sem:
                t = time.perf_counter()
                s, c = pairs[i % len(pairs)]
                await w.infer.remote(imgs[i % len(imgs)], strength=s, controlnet_scale=c, **BASE)
                lat.append(time.perf_counter() - t)

        t0 = time.perf_counter()
        await asyncio.gather(*[one(i) for i in range(n_frames)])
        return n_frames / (time.perf_counter() - t0)

    fps = asyncio.run(go())
    after = w.metrics()
    launches = after["launches"] - before["launches"]
    return fps, 1e3 * float(np.median(lat)), (after["frames"] - before["frames"]) / max(launches, 1)


def device_costs():
    """(c) and the zero-convs' kernel forms, on an engine of the real networks in this process"""
    from videosd_amd import convform as CF
    from videosd_amd import lib as L
    from videosd_amd.pipeline import PlanKey

    p = VideoSDPipeline(frame_options=True, tuning_mode="table", lanes=LANES, **MODEL)
    eng = p._engine_for(PlanKey(512, 512, 4, 4, True, False, frame_options=True), PAIRS[0], BATCH, 0, prompt=p._cache_prompt("pixar, cg", prompt="pixar, cg"))
    ops = eng.ops
    # which form the zero-convs (plain epilogue class: out_scale = 1, no residual) run in: their own table entry, or the heuristic
    tile_name = {v: k for k, v in vars(L).items() if k.startswith("TILE_") and isinstance(v, int)}
    seen = {}
    for fn, a, k in eng.program.calls:
        if fn.__name__ == "conv_group" and all(not kk for _aa, kk in a[0]) and all(aa[3].ksize == 1 for aa, _kk in a[0]):
            gkey = ops.group_key(a[0], k.get("split"))
            gent = CF.lookup(ops.tile_override, gkey)
            seen[("group of %d zero-convs" % len(a[0]),)] = "table entry %s" % (gent,) if gent is not None else "no table entry: the group's default form"
            for aa, kk in a[0]:
                key = ops.conv_key_of(aa[2], aa[3], kk)
                ent = CF.lookup(ops.tile_override, key)
                f = CF.resolve(CF.conv_call(aa[2], aa[3], **kk), ops.tile_override, ops.tune_mode, CF.flags_of(ops))
                seen[key[:3]] = (("table entry" if ent is not None else "no table entry: choose_tile ->") +
                                 f" (tile {tile_name.get(f.tile, f.tile)}, split_k {f.split_k})")
    say("zero-convs of the frame_options program (M, N, Kp) at 5 frames per launch, throughput-mode table:")
    for key, what in seen.items():
        say(f"  {key}: {what}")
    total, kinds = eng.launches_by_kind(serial=True)
    say(f"launches per replay of the 5-frame frame_options program (one-stream form): {total} {kinds}")
    # one option-entry build: a timestep tuple the cache has not seen (host wall time of the call, which ends with a synchronise)
    eng.family["option_entries"].clear()
    ms = []
    for s in (0.40, 0.46, 0.52, 0.58, 0.64, 0.72, 0.78, 0.84, 0.90, 0.96):
        ops.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(ops.stream)
        ent = eng.option_entry(s, 4)
        e1.record(ops.stream)
        ops.synchronize()
        ms.append((1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)))
    say(f"(c) one option-entry build ({ent.layout.nbytes / 1e3:.0f} KB: coefficients + two time tables of 4 steps), 10 new timestep tuples: "
        f"host {', '.join(f'{a:.2f}' for a, _b in ms)} ms (median {np.median([a for a, _b in ms]):.2f}); between events on the stream "
        f"{', '.join(f'{b:.2f}' for _a, b in ms)} ms (median {np.median([b for _a, b in ms]):.2f})")
    # one slot install
    tab, nseg = eng._seg_table(ent.layout, eng.fo_layout)
    nbytes = sum(int(r) * int(rb) for _so, _do, r, rb, _p, _f in tab.cpu().tolist())
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ops.stream)
        for i in range(200):
            ops.prompt_install(ent.buf, eng.fo_buf, tab, nseg, i % BATCH)
        e1.record(ops.stream)
        ops.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / 200)
    say(f"(c) one slot install (vsd_prompt_install, {nseg} segments, {nbytes / 1e3:.0f} KB): {', '.join(f'{v:.1f}' for v in us)} us per launch "
        f"(200 back to back between two events; median {np.median(us):.1f} us)")


def main():
    from PIL import Image

    from videosd_amd.lcm import lcm_timesteps

    if not torch.cuda.is_available():
        raise SystemExit("scripts/frame_options.py needs a GPU")
    assert {len(lcm_timesteps(s, BASE["steps"])) for s, _c in PAIRS} == {4}
    rng = np.random.default_rng(0)
    imgs = [Image.fromarray(rng.integers(0, 256, (512, 512, 3), dtype=np.uint8), "RGB") for _ in range(8)]
    workers = {False: worker(False), True: worker(True)}
    try:
        legs = [("(a) one session, frame_options off (the default program)", False, PAIRS[:1]),
                ("(a) one session, frame_options on", True, PAIRS[:1]),
                ("(b) five sessions with five pairs, frame_options off (a launch has one pair, a change drains)", False, PAIRS),
                ("(b) five sessions with five pairs, frame_options on", True, PAIRS),
                ("(b) two sessions alternating, frame_options off", False, PAIRS[:2]),
                ("(b) two sessions alternating, frame_options on", True, PAIRS[:2])]
        for name, fo, pairs in legs:  # one unrecorded pass: every leg's first stream pays for what is left to warm
            stream(workers[fo], imgs, pairs)
        res = {name: [] for name, _f, _p in legs}
        for _ in range(reps):
            for name, fo, pairs in legs:
                res[name].append(stream(workers[fo], imgs, pairs))
        say(f"5 x 4 through the class (worker process, PIL in / PIL out, {n_frames} frames per repetition, {(LANES + 1) * BATCH} outstanding), legs taking turns:")
        med = {}
        for name, _f, _p in legs:
            fps = [r[0] for r in res[name]]
            med[name] = (float(np.median(fps)), min(fps), max(fps))
            say(f"  {name}: {', '.join(f'{v:.1f}' for v in fps)} frames/s (median {med[name][0]:.1f}, spread {min(fps):.1f} .. {max(fps):.1f}); "
                f"p50 latency {', '.join(f'{r[1]:.0f}' for r in res[name])} ms; frames per launch {', '.join(f'{r[2]:.2f}' for r in res[name])}")
        for tag, (off, on) in (("(a) one session", legs[0:2]), ("(b) five sessions", legs[2:4]), ("(b) two sessions alternating", legs[4:6])):
            o, n = med[off[0]], med[on[0]]
            sep = ("separated by more than the spread of the repetitions" if (n[1] > o[2] or n[2] < o[1]) else
                   "NOT separated by more than the spread of the repetitions")
            say(f"{tag}: frame_options on / off {n[0] / o[0]:.3f} x ({sep}: on {n[1]:.1f} .. {n[2]:.1f}, off {o[1]:.1f} .. {o[2]:.1f})")
    finally:
        for w in workers.values():
            w.close()
    device_costs()
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
