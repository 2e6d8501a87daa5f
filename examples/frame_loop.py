#!/usr/bin/env python3
"""The reference's frame loop without WebRTC: a synthetic camera feeds `VideoSDPipeline.remote(...)` workers exactly the
way diffusert/server.py does (`VideoSDTrack.recv` -> `diffuse` -> `await pipelines[gpu].infer.remote(img, **options)`,
server.py:104-143), one worker process per GPU, frames sharded round-robin, drop-if-busy, newest-wins or in-order display.

  python examples/frame_loop.py --gpus 1 --fps 60 --seconds 10 --batch 3          (needs the MI355X)
  python examples/frame_loop.py --factory helpers_fake_pipeline:FakePipeline ...   (any stand-in with the same surface)
  python examples/frame_loop.py --fade-to "a charcoal sketch" --fade-frames 60 ...  (a cross-fade between two prompts, written as 60 mixes)
  python examples/frame_loop.py --color-match histogram:0.8 ...   (every output frame keeps its camera frame's colours, matched on the device)
  python examples/frame_loop.py --keep-mask banner.png ...   (black in the image: kept as the camera saw it; white: restyled; blended on the device)
  python examples/frame_loop.py --edge-blur 1.4 ...   (the edge op reads a Gaussian-blurred copy of each frame: calmer edges)
  python examples/frame_loop.py --keep-mask banner.png --mask-feather 4 ...   (the mask's hard edge feathered on the device: no seam)

Prints one JSON line: frames offered / processed / dropped, output frames per second, p50 / p95 submit->result latency.
"""
import argparse
import asyncio
import json
import os
import statistics
import sys
import time

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videosd_amd.dispatch import FrameDispatcher, RemotePipeline  # noqa: E402


def camera_frame(k: int, w: int, h: int) -> Image.Image:
    """A moving gradient with seeded noise (Sobel maximum never 0: canny_gpu.py:39 would divide by zero)."""
    rng = np.random.default_rng(k)
    yy, xx = np.mgrid[0:h, 0:w]
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) // 2 + ((xx * 2 + yy + 17 * k) % 256).astype(np.uint8)[..., None] // 2
    return Image.fromarray(a.astype(np.uint8), "RGB")


def crossfade(a: str, b: str, k: int, frames: int):
    """The prompt of frame k of a cross-fade from text `a` to text `b` over `frames` frames: a MIX of the two (`{"mix": [[a, 1 - t], [b, t]]}`,
    what `infer` takes besides a text).  The workers blend the two cached prompts on the device, one small launch per new value; nothing is
    encoded or built after the two texts are cached.  `infer` cannot tell sessions apart, so a fade is the caller's: k mixes, written out."""
    if frames <= 0 or k >= frames:
        return b
    return {"mix": [[a, 1.0 - k / frames], [b, k / frames]]}  # (k = 0 comes down to the plain prompt `a`)


async def run(args):
    cfg = dict(model=args.model, controlnet=args.controlnet)
    extra = json.loads(args.worker_config) if args.worker_config else {}
    if args.lora:  # PATH[:SCALE], up to four -> the constructor's loras (`set_lora_scale(name, value)` moves a scale live)
        loras = []
        for item in args.lora:
            path, sep, scale = item.rpartition(":")
            try:
                loras.append({"path": path, "scale": float(scale)} if sep else {"path": item})
            except ValueError:
                loras.append({"path": item})
        extra.update(loras=loras)
    if args.color_match:  # MODE[:AMOUNT] -> the constructor's color_match / color_amount (fixed mode; `set_color_match` moves the amount live)
        mode, _, amount = args.color_match.partition(":")
        extra.update(color_match=mode, color_amount=float(amount) if amount else 1.0)
    if args.keep_mask:  # FILE -> the constructor's keep_mask=True; the image itself goes to every worker below (`set_mask`, any size)
        extra.update(keep_mask=True)
    if args.edge_blur is not None:  # SIGMA -> the constructor's edge_blur (`set_edge_blur` moves it live)
        extra.update(edge_blur=args.edge_blur)
    if args.mask_feather is not None:  # SIGMA -> the constructor's mask_feather (needs --keep-mask; `set_mask_feather` moves it live)
        extra.update(mask_feather=args.mask_feather)
    workers = [RemotePipeline(factory=args.factory, batch=args.batch, device=i, **cfg, **extra) for i in range(args.gpus)]
    opts = dict(prompt=args.prompt, height=args.height, width=args.width, strength=args.strength, steps=args.steps,
                controlnet_scale=args.controlnet_scale, seed=23)
    try:
        if args.keep_mask:  # drawn over the camera picture: each worker sizes it once per frame size, as it sizes the frames
            mask = Image.open(args.keep_mask).convert("L")
            await asyncio.gather(*[w.set_mask.remote(mask) for w in workers])
        if not args.no_warmup:  # the first call of a worker builds and captures its graph (compile_model in the reference)
            await asyncio.gather(*[w.infer.remote(camera_frame(0, 640, 480), **opts) for w in workers])
        disp = FrameDispatcher(workers, mode=args.mode, depth=args.depth or args.batch * 2)
        pool = [camera_frame(i, args.cam_width, args.cam_height) for i in range(16)]  # the camera itself costs nothing
        t_sub, lat, shown = {}, [], 0
        period = 1.0 / args.fps
        t0 = time.perf_counter()

        async def display():
            nonlocal shown
            while True:
                ticket, img = await disp.next_result()
                if isinstance(img, Exception):
                    raise img
                lat.append((time.perf_counter() - t_sub[ticket]) * 1e3)
                shown += 1

        shower = asyncio.ensure_future(display())
        k = 0
        while time.perf_counter() - t0 < args.seconds:
            frame = pool[k % len(pool)]
            now = time.perf_counter()
            if args.fade_to:  # frame k of the stream carries value k of the fade
                ticket = disp.submit(frame, **dict(opts, prompt=crossfade(args.prompt, args.fade_to, k, args.fade_frames)))
            else:
                ticket = disp.submit(frame, **opts)
            if ticket is not None:
                t_sub[ticket] = now
            k += 1
            await asyncio.sleep(max(0.0, t0 + k * period - time.perf_counter()))
        while disp.pending:
            await asyncio.sleep(0.01)
        wall = time.perf_counter() - t0
        shower.cancel()
        out = {"offered": k, "processed": disp.submitted, "dropped": disp.dropped, "shown": shown, "seconds": round(wall, 2),
               "output_fps": round(shown / wall, 2), "p50_latency_ms": round(statistics.median(lat), 1) if lat else None,
               "p95_latency_ms": round(sorted(lat)[int(0.95 * (len(lat) - 1))], 1) if lat else None,
               "config": {"gpus": args.gpus, "camera_fps": args.fps, "batch": args.batch, "mode": args.mode, **opts}}
        print(json.dumps(out), flush=True)
        return out
    finally:
        for w in workers:
            w.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--fps", type=float, default=60.0, help="camera frame rate")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--batch", type=int, default=3, help="frames a worker may coalesce into one launch")
    ap.add_argument("--depth", type=int, default=0, help="frames one worker may hold (default 2 x batch)")
    ap.add_argument("--mode", default="latest", choices=["latest", "in_order"])
    ap.add_argument("--factory", default="videosd_amd.pipeline:VideoSDPipeline")
    ap.add_argument("--worker-config", default="", help="JSON of extra worker kwargs")
    ap.add_argument("--model", default="SimianLuo/LCM_Dreamshaper_v7")
    ap.add_argument("--controlnet", default="lllyasviel/control_v11p_sd15_canny")
    ap.add_argument("--prompt", default="pixar, cg")
    ap.add_argument("--fade-to", dest="fade_to", default="", help="cross-fade from --prompt to this prompt, as prompt mixes")
    ap.add_argument("--fade-frames", dest="fade_frames", type=int, default=60, help="frames the cross-fade takes")
    ap.add_argument("--lora", action="append", default=[], metavar="PATH[:SCALE]",
                    help="a LoRA adapter file (safetensors) fused on the device at SCALE (default 1.0); up to four")
    ap.add_argument("--color-match", dest="color_match", default="", metavar="MODE[:AMOUNT]",
                    help="histogram or meanstd, and an amount in [0, 1] (default 1): transfer each camera frame's colours onto its output frame")
    ap.add_argument("--keep-mask", dest="keep_mask", default="", metavar="FILE",
                    help="an image of any size, read as gray: 0 / black is kept as the camera saw it, 255 / white is restyled, values between blend")
    ap.add_argument("--edge-blur", dest="edge_blur", type=float, default=None, metavar="SIGMA",
                    help="sigma in [0, 10] of a Gaussian blur ahead of the edge op, on the device: the ControlNet's edges come from the calmed copy")
    ap.add_argument("--mask-feather", dest="mask_feather", type=float, default=None, metavar="SIGMA",
                    help="sigma in [0, 10] of a Gaussian blur over the keep mask, on the device (needs --keep-mask)")
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--strength", type=float, default=0.6)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--controlnet-scale", dest="controlnet_scale", type=float, default=1.0)
    ap.add_argument("--cam-width", dest="cam_width", type=int, default=640)
    ap.add_argument("--cam-height", dest="cam_height", type=int, default=480)
    ap.add_argument("--no-warmup", action="store_true")
    return asyncio.run(run(ap.parse_args(argv)))


if __name__ == "__main__":
    main()
