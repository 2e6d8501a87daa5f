"""Camera-sized frames through the drop-in class, with the crop + LANCZOS resize on the host (PIL, the reference's way,
videopipeline.py:92-107) and on the device (`device_resize=True`, csrc/resample.hip), in ONE process run.

bench.py's drop-in legs feed frames that already are 512 x 512, for which PIL's resize is a copy; a WebRTC camera sends 1280 x 720
or 1920 x 1080.  This streams N seeded frames of each size through `VideoSDPipeline.remote` at the bench's operating point
(512 x 512, 4 steps, ControlNet, strength 0.6; 5 frames per launch x 4 lanes, and one frame at a time), alternating a worker with
device_resize off and one with it on, next to the already-sized stream, and prints frames/s, p50 latency and the worker's
`crop_resize` host milliseconds per frame.

    python scripts/camera_frames.py [--frames 320] [--singles 280] [--reps 2] [--sizes 512x512,1280x720,1920x1080]

With --op it times the kernel alone instead (a few hundred launches of the 1280 x 720 and 1920 x 1080 resample on one stream; run it
under `rocprofv3 --kernel-trace --stats -- python scripts/camera_frames.py --op` for the per-kernel times)."""
import argparse
import asyncio
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H = W = 512
OPTS = dict(prompt="pixar, cg", height=H, width=W, strength=0.6, steps=4, controlnet_scale=1.0, seed=23)


def camera_frames(n, h, w, seed):
    """seeded noise blended with a moving gradient (bench.py's synthetic frames, at a camera's size)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        grad = ((xx * 2 + yy + 17 * i) % 256).astype(np.uint8)[..., None]
        out.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8) // 2 + grad // 2)
    return out


def op_times(reps):
    import torch

    from videosd_amd.ops import HipOps

    ops = HipOps(0)
    for h, w in ((720, 1280), (1080, 1920), (2160, 3840)):
        src = torch.from_numpy(camera_frames(1, h, w, 5)[0]).to(ops.device)
        dst = torch.zeros(H, W, 3, dtype=torch.uint8, device=ops.device)
        box = ops.center_crop_box(w, h, W, H)
        for _ in range(10):
            ops.resample_rgb(src, h, w, 3 * w, box, dst, H, W)
        ops.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ops.stream)
        for _ in range(reps):
            ops.resample_rgb(src, h, w, 3 * w, box, dst, H, W)
        e1.record(ops.stream)
        ops.synchronize()
        print(json.dumps({"op": "resample_rgb", "src": f"{w}x{h}", "box": box, "dst": f"{W}x{H}", "launches": reps,
                          "us_per_frame_back_to_back": round(1e3 * e0.elapsed_time(e1) / reps, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=320, help="frames per stream measurement")
    ap.add_argument("--singles", type=int, default=280, help="frames sent one at a time (p50 latency; fills the worker's window of stage times)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--sizes", default="512x512,1280x720,1920x1080")
    ap.add_argument("--op", action="store_true")
    a = ap.parse_args()
    if a.op:
        return op_times(300)
    from PIL import Image

    from videosd_amd.pipeline import VideoSDPipeline

    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    imgs = {(w, h): [Image.fromarray(f, "RGB") for f in camera_frames(8, h, w, 1234 + w)] for w, h in sizes}
    slot = max(w * h * 3 for w, h in sizes)  # (the default slot, 3 MiB, holds 1280 x 720; 1920 x 1080 would travel pickled)
    workers = {}
    try:
        for mode in ("host", "device"):
            workers[mode] = VideoSDPipeline.remote(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0,
                                                   batch=a.batch, lanes=a.lanes, shm_slots=(a.lanes + 1) * a.batch + 4, shm_slot_bytes=slot,
                                                   call_timeout=600.0, device_resize=(mode == "device"))
            workers[mode].method("warm_up")(batches=tuple(range(1, a.batch + 1)), lanes=a.lanes, **OPTS)
        # the two paths return the same picture (the GPU tests assert it byte for byte; here: the frames this run measures)
        for (w, h), ims in imgs.items():
            same = np.array_equal(np.asarray(workers["host"].infer(ims[0], **OPTS)), np.asarray(workers["device"].infer(ims[0], **OPTS)))
            print(json.dumps({"check": f"{w}x{h}", "device_resize_gives_the_host_paths_bytes": bool(same)}), flush=True)

        async def stream(wk, ims, n, depth):
            sem = asyncio.Semaphore(depth)

            async def one(i):
                async with sem:
                    await wk.infer.remote(ims[i % len(ims)], **OPTS)

            t0 = time.perf_counter()
            await asyncio.gather(*[one(i) for i in range(n)])
            return n / (time.perf_counter() - t0)

        rows = []
        for rep in range(a.reps):
            for (w, h), ims in imgs.items():
                for mode in ("host", "device"):
                    wk = workers[mode]
                    fps = asyncio.run(stream(wk, ims, a.frames, (a.lanes + 1) * a.batch))
                    lat = []
                    for i in range(a.singles):
                        t0 = time.perf_counter()
                        wk.infer(ims[i % len(ims)], **OPTS)
                        lat.append((time.perf_counter() - t0) * 1e3)
                    st = (wk.metrics().get("pipeline") or {}).get("stage_ms_p50") or {}
                    row = {"rep": rep, "input": f"{w}x{h}", "resize": mode, "stream_fps": round(fps, 2), "one_at_a_time_p50_ms": round(statistics.median(lat), 2),
                           "one_at_a_time_fps": round(1e3 / statistics.median(lat), 2), "crop_resize_host_ms_per_frame": st.get("crop_resize"),
                           "upload_enqueue_host_ms_per_frame": st.get("upload_enqueue"), "gpu_ms_per_frame": st.get("gpu")}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        # best of the repetitions per (input, path), and device / host
        print(f"\n{'input':>10} {'resize':>7} {'stream f/s':>11} {'single p50 ms':>14} {'crop_resize ms':>15}")
        best = {}
        for r in rows:
            k = (r["input"], r["resize"])
            if k not in best or r["stream_fps"] > best[k]["stream_fps"]:
                best[k] = r
        for (inp, mode), r in best.items():
            print(f"{inp:>10} {mode:>7} {r['stream_fps']:>11.2f} {r['one_at_a_time_p50_ms']:>14.2f} {r['crop_resize_host_ms_per_frame']!s:>15}")
        sized = best.get((f"{W}x{H}", "device"))
        for (inp, mode), r in best.items():
            if mode == "device" and (inp, "host") in best:
                hst = best[(inp, "host")]
                print(json.dumps({"input": inp, "stream_fps_device_over_host": round(r["stream_fps"] / hst["stream_fps"], 3),
                                  "one_at_a_time_fps_device_over_host": round(r["one_at_a_time_fps"] / hst["one_at_a_time_fps"], 3),
                                  "stream_fps_device_over_already_sized": round(r["stream_fps"] / sized["stream_fps"], 3) if sized else None}), flush=True)
    finally:
        for wk in workers.values():
            wk.close()


if __name__ == "__main__":
    main()
