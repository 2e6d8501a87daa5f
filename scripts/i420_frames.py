"""Camera-sized frames through the drop-in class as RGB PIL images and as I420 frames (`frames.I420Frame`), in ONE process run.

A WebRTC loop never holds RGB: a decoded frame is planar YUV 4:2:0 and the encoder takes it again.  This streams the same seeded
pictures through ONE `VideoSDPipeline.remote(device_resize=True)` worker at the bench's operating point (512 x 512, 4 steps,
ControlNet, strength 0.6; 5 frames per launch x 4 lanes, and one frame at a time), alternating two legs and repeating them:
  rgb   PIL RGB frames -- the best the commit before this path could do, and this leg is GIVEN RGB for free: the server's two
        libswscale conversions (`frame.to_image()`, `VideoFrame.from_image`) are not in it, so the comparison understates the gain;
  i420  the same pictures as I420Frames: planes through shared memory, converted on the device both ways (csrc/yuv.hip).
Prints frames/s, one-at-a-time p50, the worker's host milliseconds per stage, the bytes uploaded and downloaded per frame (counted
by the worker, not timed) and the parent's slot-write / slot-read seconds per frame.

    python scripts/i420_frames.py [--frames 320] [--singles 280] [--reps 2] [--sizes 1280x720,1920x1080]

--op times the conversions alone (300 back-to-back launches per shape on one stream, HIP events; run it under
`rocprofv3 --kernel-trace --stats -- python scripts/i420_frames.py --op` for the per-kernel times, no counters in that run);
--trace-csv FILE groups such a run's kernel_trace.csv by kernel and grid and prints median microseconds next to the bytes each
kernel has to move."""
import argparse
import asyncio
import ctypes as C
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


def crop_box(w, h):
    from videosd_amd import lib as L

    b = (C.c_int * 4)()
    assert L.load().vsd_center_crop_box(w, h, W, H, b) == 0
    return tuple(b)


def op_times(reps):
    import torch

    from videosd_amd.frames import I420Frame
    from videosd_amd.ops import HipOps

    ops = HipOps(0)

    def timed(fn):
        for _ in range(10):
            fn()
        ops.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ops.stream)
        for _ in range(reps):
            fn()
        e1.record(ops.stream)
        ops.synchronize()
        return round(1e3 * e0.elapsed_time(e1) / reps, 2)

    for h, w in ((720, 1280), (1080, 1920)):
        f = I420Frame.from_rgb(camera_frames(1, h, w, 5)[0])
        l, t, r, b = crop_box(w, h)
        rw, rh = r - l, b - t  # (even left / top edges for both sizes: the uploaded rectangle is the box)
        dy = torch.from_numpy(np.ascontiguousarray(f.y[t:b, l:r])).to(ops.device)
        du = torch.from_numpy(np.ascontiguousarray(f.u[t // 2:(b + 1) // 2, l // 2:(r + 1) // 2])).to(ops.device)
        dv = torch.from_numpy(np.ascontiguousarray(f.v[t // 2:(b + 1) // 2, l // 2:(r + 1) // 2])).to(ops.device)
        rgb = torch.zeros(rh, rw, 3, dtype=torch.uint8, device=ops.device)
        dst = torch.zeros(H, W, 3, dtype=torch.uint8, device=ops.device)
        conv = lambda: ops.i420_to_rgb(dy, rw, du, dv, du.shape[1], 0, 0, rh, rw, rgb, rw * 3)  # noqa: E731
        res = lambda: ops.resample_rgb(rgb, rh, rw, rw * 3, (0, 0, rw, rh), dst, H, W)  # noqa: E731
        print(json.dumps({"op": "i420_to_rgb", "src": f"{w}x{h}", "rect": f"{rw}x{rh}", "launches": reps, "us_per_frame_back_to_back": timed(conv),
                          "bytes_read": rw * rh * 3 // 2, "bytes_written": rw * rh * 3}), flush=True)
        print(json.dumps({"op": "resample_rgb", "src": f"{w}x{h}", "rect": f"{rw}x{rh}", "dst": f"{W}x{H}", "launches": reps,
                          "us_per_frame_back_to_back": timed(res)}), flush=True)
        print(json.dumps({"op": "i420_to_rgb + resample_rgb", "src": f"{w}x{h}", "launches": reps,
                          "us_per_frame_back_to_back": timed(lambda: (conv(), res()))}), flush=True)
    out = torch.from_numpy(camera_frames(1, H, W, 6)[0]).to(ops.device)
    planes = torch.zeros(H * W * 3 // 2, dtype=torch.uint8, device=ops.device)
    back = lambda: ops.rgb_to_i420(out, H, W, planes[:H * W], planes[H * W:H * W * 5 // 4], planes[H * W * 5 // 4:])  # noqa: E731
    print(json.dumps({"op": "rgb_to_i420", "src": f"{W}x{H}", "launches": reps, "us_per_frame_back_to_back": timed(back),
                      "bytes_read": H * W * 3, "bytes_written": H * W * 3 // 2}), flush=True)


def trace_table(path):
    """median / min microseconds per (kernel, grid) of a rocprofv3 kernel_trace.csv, next to the bytes the kernel must move"""
    import collections
    import csv

    moved = {}
    for w, h in ((1280, 720), (1920, 1080)):
        l, t, r, b = crop_box(w, h)
        moved[("i420_to_rgb", (r - l + 3) // 4, (b - t + 1) // 2)] = f"{(r - l) * (b - t) * 9 // 2} B ({(r - l) * (b - t) * 3 // 2} in, {(r - l) * (b - t) * 3} out)"
    moved[("rgb_to_i420", W // 4, H // 2)] = f"{H * W * 9 // 2} B ({H * W * 3} in, {H * W * 3 // 2} out)"
    groups = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r.get("Kernel_Name", "")
        if not any(k in name for k in ("i420", "resample_")):
            continue
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:40]
        key = (short, r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Grid_Size_Y", ""))
        groups[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for key, us in sorted(groups.items()):
        note = ""
        for (k, gx, gy), txt in moved.items():  # (grid sizes in the trace are work-items: strips rounded up to the 64 x 4 block)
            if k in key[0] and key[1] and int(key[1]) == -(-gx // 64) * 64 and key[2] and int(key[2]) == -(-gy // 4) * 4:
                b = int(txt.split(" ")[0])
                note = f" must move {txt}: {b / statistics.median(us) / 1e3:.0f} GB/s at the median"
        print(f"{key} n={len(us)} median_us={statistics.median(us):.2f} min_us={min(us):.2f}{note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=320, help="frames per stream measurement")
    ap.add_argument("--singles", type=int, default=280, help="frames sent one at a time (p50 latency; fills the worker's window of stage times)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--trace-csv")
    a = ap.parse_args()
    if a.trace_csv:
        return trace_table(a.trace_csv)
    if a.op:
        return op_times(300)
    if a.reps < 2:
        raise SystemExit("--reps: at least 2 (the spread between repetitions of a leg is what the legs are compared against)")
    from PIL import Image

    from videosd_amd.frames import I420Frame
    from videosd_amd.pipeline import VideoSDPipeline

    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    # the SAME pictures on both legs: a seeded frame is taken to I420 once (host loop of the contract), the rgb leg gets its conversion back
    frames = {}
    for w, h in sizes:
        yuv = [I420Frame.from_rgb(f) for f in camera_frames(8, h, w, 1234 + w)]
        frames[(w, h)] = {"i420": yuv, "rgb": [Image.fromarray(f.to_rgb(), "RGB") for f in yuv]}
    slot = max(w * h * 3 for w, h in sizes)  # (RGB 1920 x 1080 does not fit the default 3 MiB slot; the I420 frame would)
    wk = VideoSDPipeline.remote(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", device=0, batch=a.batch,
                                lanes=a.lanes, shm_slots=(a.lanes + 1) * a.batch + 4, shm_slot_bytes=slot, call_timeout=600.0, device_resize=True)
    try:
        wk.method("warm_up")(batches=tuple(range(1, a.batch + 1)), lanes=a.lanes, **OPTS)
        for (w, h), fr in frames.items():
            got, ref = wk.infer(fr["i420"][0], **OPTS), wk.infer(fr["rgb"][0], **OPTS)
            same = isinstance(got, I420Frame) and got == I420Frame.from_rgb(np.asarray(ref))
            print(json.dumps({"check": f"{w}x{h}", "the_i420_leg_gives_the_contract_around_the_rgb_legs_bytes": bool(same)}), flush=True)

        async def stream(ims, n, depth):
            sem = asyncio.Semaphore(depth)

            async def one(i):
                async with sem:
                    await wk.infer.remote(ims[i % len(ims)], **OPTS)

            t0 = time.perf_counter()
            await asyncio.gather(*[one(i) for i in range(n)])
            return n / (time.perf_counter() - t0)

        rows = []
        for rep in range(a.reps):
            for (w, h), fr in frames.items():
                for leg in ("rgb", "i420"):
                    ims = fr[leg]
                    before = dict(wk.host_s)
                    fps = asyncio.run(stream(ims, a.frames, (a.lanes + 1) * a.batch))
                    lat = []
                    for i in range(a.singles):
                        t0 = time.perf_counter()
                        wk.infer(ims[i % len(ims)], **OPTS)
                        lat.append((time.perf_counter() - t0) * 1e3)
                    n = max(1, wk.host_s["frames"] - before["frames"])
                    met = wk.metrics().get("pipeline") or {}
                    st = met.get("stage_ms_p50") or {}
                    bpf = met.get("io_bytes_per_frame") or {}  # (the worker's own count of what it handed to the copies, last launch)
                    row = {"rep": rep, "input": f"{w}x{h}", "leg": leg, "stream_fps": round(fps, 2), "one_at_a_time_p50_ms": round(statistics.median(lat), 2),
                           "crop_resize_ms": st.get("crop_resize"), "upload_enqueue_ms": st.get("upload_enqueue"), "wait_download_ms": st.get("wait_download"),
                           "to_pil_or_to_i420_ms": st.get("to_pil" if leg == "rgb" else "to_i420"), "gpu_ms": st.get("gpu"),
                           "upload_bytes": bpf.get("up"), "download_bytes": bpf.get("down"),
                           "parent_slot_write_us": round(1e6 * (wk.host_s["slot_write"] - before["slot_write"]) / n, 1),
                           "parent_slot_read_us": round(1e6 * (wk.host_s["slot_read"] - before["slot_read"]) / n, 1)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        print(f"\n{'input':>10} {'leg':>5} {'stream f/s per rep':>24} {'spread':>7} {'single p50 ms':>14} {'up B':>9} {'down B':>8} {'slot wr us':>11} {'slot rd us':>11}")
        by = {}
        for r in rows:
            by.setdefault((r["input"], r["leg"]), []).append(r)
        for (inp, leg), rs in by.items():
            f = [r["stream_fps"] for r in rs]
            print(f"{inp:>10} {leg:>5} {' '.join('%.2f' % v for v in f):>24} {max(f) - min(f):>7.2f} {statistics.median(r['one_at_a_time_p50_ms'] for r in rs):>14.2f} "
                  f"{rs[0]['upload_bytes']:>9} {rs[0]['download_bytes']:>8} {statistics.median(r['parent_slot_write_us'] for r in rs):>11.1f} "
                  f"{statistics.median(r['parent_slot_read_us'] for r in rs):>11.1f}")
        for (w, h) in sizes:
            inp = f"{w}x{h}"
            fa, fb = [r["stream_fps"] for r in by[(inp, "rgb")]], [r["stream_fps"] for r in by[(inp, "i420")]]
            spread_a = max(fa) - min(fa)
            print(json.dumps({"input": inp, "rgb_stream_fps_mean": round(statistics.mean(fa), 2), "i420_stream_fps_mean": round(statistics.mean(fb), 2),
                              "rgb_spread": round(spread_a, 2), "i420_spread": round(max(fb) - min(fb), 2),
                              "i420_not_below_rgb_by_more_than_the_rgb_spread": bool(statistics.mean(fb) >= statistics.mean(fa) - spread_a)}), flush=True)
    finally:
        wk.close()


if __name__ == "__main__":
    main()
